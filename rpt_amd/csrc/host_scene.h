// host_scene.h — host side of rptgpu_scene_create: kd-tree construction by the reference rule
// and flattening of the boundary's POD scene description into the device layout.
#pragma once
#include <string>
#include <vector>

#include "../../include/rpt_gpu.h"
#include "device_types.h"

namespace rpthost {

struct Box {
  double lo[3], hi[3];
};

struct KdBuild {
  std::vector<rptdev::KdNode> nodes;
  std::vector<uint32_t> refs;
  uint32_t max_depth = 0;
  bool regular = true; // every split plane lies inside its node's cell
};

// KdTree::new (kdtree.rs:108-119) -> construct (kdtree.rs:235-345), flattened.
// threads <= 0: std::thread::hardware_concurrency() (RPTGPU_BUILD_THREADS overrides), at most 32; the tree is the same
// for any thread count (host_scene.cpp, splice)
void kd_build(const std::vector<Box>& boxes, KdBuild& out, int threads = 0);

// The same tree, node for node, built on HIP device `device` (kdbuild.hip: events sorted once per axis, then one round
// of scans and stable scatters per tree level).  Returns false — `why` says why — when it cannot be used (fewer than 16
// primitives, non-finite boxes, a HIP error, a tree deeper than the device stack): the caller builds on the host then.
bool kd_build_device(const std::vector<Box>& boxes, KdBuild& out, int device, std::string& why);

// scene hand-off options: trees of at least device_build_min primitives are built on the device (0: never)
struct BuildOptions {
  int device = -1;
  size_t device_build_min = 0;
  int build_threads = 0; // RptSceneOptions::build_threads: 0 = the usable cores
};

// The tree over `boxes` as scene creation builds it: on the device when `build` names one and there are at least
// device_build_min boxes and the device builder takes them, else on the host (the same tree); -> built on the device
bool build_kd(const std::vector<Box>& boxes, const BuildOptions* build, KdBuild& kb);
// What creation derives from a built tree and its primitives' boxes, into `t`: num_prims, sample_zone, regular,
// split_range_ok, root_leaf / root_first and the bounds (BoundingBox::merge folded in index order, kdtree.rs:110-113).
// One source for rptgpu_scene_create and rptgpu_scene_set_mesh; node_base, ref_base, prim_base and the leaf grid are the caller's.
void derive_tree(const KdBuild& kb, const std::vector<Box>& boxes, rptdev::Tree& t);

// ---- what the flattening derives from the objects' placements and materials.  One source for rptgpu_scene_create and
// the live updates of a handle (rptgpu_scene_set_objects / _lights, api_scene.cpp), so an updated handle holds the bits a
// fresh one of the updated scene would.

// per top-level object, fixed at creation (its geometry does not change under an update): what its world box and the
// object filter need besides the placement
struct ObjectGeom {
  Box local;           // Bounded::bounding_box before Transformed (shape.rs:153-176 transforms it)
  bool bounded = false; // not a Plane
  bool sliver = false;  // a mesh with an ill-conditioned triangle: never filtered (fill_object_boxes, host_scene.cpp)
};

// derived from the top-level objects' world boxes
struct ObjectBounds {
  // flat scenes' object filter (kernels/paths_flat.inc flat_query_filtered): one conservative box per TOP-LEVEL object on a
  // grid over all bounded ones; bit k of obj_always: object k is never filtered.  obj_filter_ok: every object is of a
  // kind the filtered walk handles (sphere, cube, plane, mesh) and there are at most 64 of them
  std::vector<rptdev::LeafBox> obj_lbox;
  double obj_grid[12] = {0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0}; // qlo[3], qscale[3], bounds[6]
  uint64_t obj_always = ~0ull;
  bool obj_filter_ok = false;
  // union of the world-space boxes of the bounded top-level objects (planes have none): the grid of the path re-order's
  // sort key (kernels/wf_sort_key.inc ray_sort_key); ok: there is at least one and it is finite and not flat
  double scene_bounds[6] = {0, 0, 0, 1, 1, 1};
  bool scene_bounds_ok = false;
};

// Transformed's five fields (shape.rs:101-124) into `in`; zeros when the shape is not transformed
void set_transform(rptdev::Inst& in, const RptShape& s);
// Material -> its device record; refuses (RPTGPU_E_INVALID_ARGUMENT, `err` names object `i`) a material whose specular lobe
// probability lies outside [0, 1]
int convert_material(const RptMaterial& s, uint64_t i, rptdev::Material& m, std::string& err);
// a light's record without its shape (Light::inst is left -1); RPTGPU_E_INVALID_ARGUMENT for an unknown kind
int convert_light(const RptLight& l, rptdev::Light& dl, std::string& err);
// the world box of a top-level object: Bounded::bounding_box through its placement `in` (meaningful when g.bounded)
Box world_box(const ObjectGeom& g, const rptdev::Inst& in);
// The pixels whose pinhole camera rays can hit something inside `world` (an object's bounding box), as an inclusive
// rectangle rect = {x0, x1, y0, y1} of a width x height frame (x0 > x1: none); false when no rectangle can be given
// (a lens, a corner not in front of the eye, values that are not finite, a frame beyond 65535 pixels a side)
bool pinhole_screen_rect(const Box& world, const rptdev::Camera& cam, uint32_t width, uint32_t height, uint32_t rect[4]);
// the object filter's tables and the scene bounds of the top-level objects insts[0, geom.size()), from scratch
void fill_object_boxes(const std::vector<rptdev::Inst>& insts, const std::vector<ObjectGeom>& geom, ObjectBounds& out);

struct FlatScene : ObjectBounds {
  std::vector<rptdev::Inst> insts;
  std::vector<rptdev::Tree> trees;
  std::vector<uint32_t> tree_depth; // per tree: depth of its deepest leaf
  std::vector<uint8_t> tree_kids;   // per tree (GROUP): bit 0 a child is a MESH, bit 1 a GROUP sits somewhere below it
  uint32_t generic_levels = 0, generic_frames = 0; // heights of rpt_tree_generic's columns that hold any object of the scene
  std::vector<rptdev::KdNode> nodes;
  std::vector<uint32_t> refs;
  std::vector<rptdev::Tri> tris;
  std::vector<rptdev::TriX> trix; // by triangle index (host-side staging only)
  std::vector<rptdev::TriX> lrec; // by refs[] position: what the device reads
  std::vector<rptdev::LeafBox> lbox; // by refs[] position: conservative boxes in front of the exact test
  std::vector<rptdev::Material> materials;
  std::vector<rptdev::Light> lights;
  std::vector<double> env_texels;
  double env_color[3] = {0, 0, 0};
  uint32_t env_width = 0, env_height = 0;
  int32_t env_kind = 0;
  int32_t num_objects = 0;
  int32_t num_shadow_lights = 0;
  uint32_t max_tree_depth = 0;
  std::vector<ObjectGeom> obj_geom; // per top-level object (the object filter and scene bounds: ObjectBounds above)
  uint32_t num_top_insts = 0;       // insts[0, num_top_insts): the objects, then the Light::Object shapes in light order
  uint32_t trees_built_on_device = 0; // how many of the trees kd_build_device made (diagnostics)
  bool nested_mesh = false; // some KdTree<Box<dyn Bounded>> child is a Mesh, a MonomialSurface or another group:
                            // the scene needs the extended kernel builds
};

// returns RPTGPU_OK or an error code; `err` explains
int flatten_scene(const RptScene& scene, FlatScene& out, std::string& err, const BuildOptions* build = nullptr);

} // namespace rpthost
