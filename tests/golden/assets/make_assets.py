"""Writes the asset fixtures of this directory from a checkout of the reference's examples/ directory:

    python tests/golden/assets/make_assets.py <reference>/examples

teapot.obj, wine_glass.obj, rustacean.obj, monomial.obj and cylinder.stl are stored whole, xz-compressed.  pegasus.zip
(7 MB of OBJ inside) is stored as a zip of the same name holding the first PEGASUS_FACES faces of its pegasus.obj with
the vertices and normals they use (its faces are `f i//i j//j k//k` over vertices in file order, so the first n faces use
the first 3n of each)."""
import lzma
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
WHOLE = ("teapot.obj", "wine_glass.obj", "rustacean.obj", "monomial.obj", "cylinder.stl")
PEGASUS_FACES = 1024


def main():
    src = sys.argv[1]
    for name in WHOLE:
        with open(os.path.join(src, name), "rb") as f, lzma.open(os.path.join(HERE, name + ".xz"), "wb", preset=9) as g:
            g.write(f.read())
    keep, nf = [], 0
    with zipfile.ZipFile(os.path.join(src, "pegasus.zip")) as z:
        counts = {"v": 0, "vn": 0}
        for line in z.read("pegasus.obj").decode().splitlines(keepends=True):
            tok = line.split(" ", 1)[0]
            if tok in counts:
                counts[tok] += 1
                if counts[tok] <= 3 * PEGASUS_FACES:
                    keep.append(line)
            elif tok == "f":
                nf += 1
                if nf <= PEGASUS_FACES:
                    assert all(int(i) <= 3 * PEGASUS_FACES for v in line.split()[1:] for i in v.split("/") if i), line
                    keep.append(line)
            else:
                keep.append(line)
    info = zipfile.ZipInfo("pegasus.obj", date_time=(2020, 11, 30, 0, 41, 0))
    with zipfile.ZipFile(os.path.join(HERE, "pegasus.zip"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        z.writestr(info, "".join(keep), compress_type=zipfile.ZIP_DEFLATED)


if __name__ == "__main__":
    main()
