/*
 * srh.h -- C ABI of the MI355X-native ("hip") backend for DiffRend's render(scene) hot path.
 *
 * The reference project (fmannan/surf_renderer) has no FFI for this path: each backend is a Python
 * module exposing `render(scene) -> dict` (diffrend/numpy/renderer.py:204-272,
 * diffrend/torch/renderer.py:136-355).  This header is the boundary a `--use hip` backend binds
 * instead: one call per frame per GPU, plain pointers and sizes, no torch / numpy types.  The
 * Python mirror of the reference interface lives in surf_renderer_amd/renderer.py and calls these
 * entry points through ctypes (see INTEGRATION.md for the stub a maintainer would add).
 *
 * Conventions
 *   - Every device buffer is allocated and freed by the caller.  The library keeps no device memory
 *     and no state between calls; all work is enqueued on the stream that is passed in and no entry
 *     point synchronises.  One documented exception, srh_render_views and srh_render_views_bwd: their per-view
 *     descriptors go through pinned staging buffers and a ring of four batches in constant memory that the library
 *     owns PER DEVICE (created on first use of a device, kept until the process ends, one mutex per
 *     device; calls on different devices do not share anything).  A call waits on the host only if the
 *     slot it reuses is still in flight, four calls back; it must be made with the stream's device
 *     current, and it cannot be stream-captured (srh_render_fwd can).
 *   - Thread safety: every entry point may be called from any thread; srh_last_error() is per thread.
 *     Concurrent srh_render_views / srh_render_views_bwd calls on one device serialise on that device's mutex.
 *   - Arrays use the reference's layouts (docs/scene_description.md, numpy/renderer.py:299-358):
 *     homogeneous 4-vectors, points w = 1, directions / normals w = 0, row-major, float32 on the
 *     device; index arrays are int32.
 *   - Primitive numbering is the reference's: segments in scene['objects'] dict order, running offset
 *     (numpy/renderer.py:172-201).  The lowest global index wins exact depth ties (np.argmin, :223).
 *   - Return value: 0 on success, a positive hipError_t, or a negative SRH_E_* code.  No C++ exception
 *     crosses the boundary; srh_last_error() returns a thread-local message for the last failure.
 */
#ifndef SRH_H
#define SRH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRH_ABI_VERSION 12
#define SRH_MAX_SEGMENTS 4
#define SRH_MAX_LIGHTS 64

/* primitive types: keys of scene['objects'] (numpy/renderer.py:133-137) */
enum { SRH_PRIM_DISK = 0, SRH_PRIM_PLANE = 1, SRH_PRIM_SPHERE = 2, SRH_PRIM_TRIANGLE = 3 };

/* error codes (negative; positive values are hipError_t) */
enum {
  SRH_OK = 0,
  SRH_E_NULL = -1,        /* a required pointer is NULL */
  SRH_E_RANGE = -2,       /* a count / row range / viewport is out of range */
  SRH_E_TYPE = -3,        /* unknown primitive type or mode */
  SRH_E_WORKSPACE = -4,   /* workspace too small or misaligned */
  SRH_E_CAMERA = -5,      /* degenerate camera (eye == at, zero up, w conventions violated) */
  SRH_E_NOT_APPLICABLE = -6 /* a measurement helper was asked about data that frames of this kind do not have */
};

/* render modes (SrhParams.mode) -- all modes produce bit-identical outputs */
enum {
  SRH_MODE_AUTO = 0,      /* the fastest exact path */
  SRH_MODE_EXACT = 1,     /* every (pixel, primitive) pair through the fp64 intersection (checker mode) */
  SRH_MODE_FAST = 2,      /* all pairs: fp32 conservative screen-space reject + fp64 confirmation of survivors */
  SRH_MODE_BINNED = 3     /* primitives binned to 16x16-pixel tiles by their screen bounding box, then as FAST */
};

/* scene['camera'] (numpy/renderer.py:145-169, numpy/ops.py:88-115).  Host memory, float64.
 * The caller applies the reference's float32 detour for list-typed at/up before filling this (see up_is_unit). */
typedef struct SrhCamera {
  double eye[4];          /* w must be 1 */
  double at[4];
  double up[4];           /* w must be 0 */
  double fovy;            /* radians */
  double focal_length;
  double near_clip;       /* valid hit: near <= t <= far on Euclidean ray distance (:219) */
  double far_clip;
  int32_t viewport[4];    /* x0, y0, x1, y1; W = x1 - x0, H = y1 - y0 */
  int32_t ortho;          /* 1: orthographic projection (torch/utils.py:461-468) -- SRH_SHADING_TORCH only (the numpy
                             backend has none); forward (all pairs in fp64), backward and srh_render_views; 0: perspective */
  int32_t up_is_unit;     /* 1: `up` is already the camera's y axis and is used as given.  The reference normalises a
                             list-typed `up` in float32 arithmetic (numpy/ops.py:99,109), which the host repeats with
                             the same numpy call before filling this; 0: y = up / |up| in float64 */
} SrhCamera;

/* one entry of scene['objects']: a batch of primitives of one type (device pointers) */
typedef struct SrhSegment {
  int32_t type;                 /* SRH_PRIM_* */
  int32_t count;
  const float* pos;             /* (count,4)   disk, plane, sphere */
  const float* normal;          /* (count,4)   disk, plane, triangle (never recomputed from vertices, :107) */
  const float* radius;          /* (count)     disk, sphere */
  const float* face;            /* (count,3,4) triangle */
  const int32_t* material_idx;  /* (count) */
} SrhSegment;

typedef struct SrhObjects {
  int32_t n_segments;           /* <= SRH_MAX_SEGMENTS, scene['objects'] dict order */
  SrhSegment seg[SRH_MAX_SEGMENTS];
} SrhObjects;

/* scene['lights'] + scene['colors'] (numpy/renderer.py:234-237) */
typedef struct SrhLights {
  int32_t n_lights;             /* <= SRH_MAX_LIGHTS */
  int32_t n_colors;
  const float* pos;             /* (n_lights,4) device */
  const int32_t* color_idx;     /* (n_lights)   device, rows of `colors` */
  const float* colors;          /* (n_colors,3) device */
  const float* attenuation;     /* (n_lights,3) device, (kc, kl, kq); SRH_SHADING_TORCH only, NULL = (1,0,0) */
  const float* ambient;         /* (3) device; SRH_SHADING_TORCH only, NULL = 0 */
} SrhLights;

/* scene['materials'] (numpy/renderer.py:245) */
typedef struct SrhMaterials {
  int32_t n_materials;
  const float* albedo;          /* (n_materials,3) device */
  const float* coeffs;          /* (n_materials,3) device, (diffuse, specular, shininess); SRH_SHADING_TORCH only,
                                   NULL = (1,0,0) */
} SrhMaterials;

/* Which of the reference's two differentiable-renderer semantics a frame follows (SrhParams.shading). */
enum {
  SRH_SHADING_NUMPY = 0,  /* diffrend/numpy/renderer.py: Lambert, clip after the light sum, +inf background, the
                             reference's non-orthonormal camera basis and 4-D normalisation */
  SRH_SHADING_TORCH = 1   /* diffrend/torch/renderer.py:82-125,136-355: attenuation, per-light relu, specular, ambient,
                             double_sided, use_quartic, orthonormal camera basis, far+1 background */
};

typedef struct SrhParams {
  int32_t row0, row1;           /* render image rows [row0,row1) of the camera's H rows; the output
                                   buffers hold only those rows (multi-GPU row slabs) */
  int32_t mode;                 /* SRH_MODE_* */
  int32_t tonemap_gamma;        /* 1: image <- image ** gamma  (scene has a 'tonemap' entry, :262) */
  double gamma;
  int32_t shading;              /* SRH_SHADING_* */
  int32_t double_sided;         /* torch shading: flip the normal towards the viewer (torch/renderer.py:107-112) */
  int32_t use_quartic;          /* torch shading: attenuation uses d^4 instead of d^2 (torch/renderer.py:92) */
  int32_t waves_per_tile;       /* binned mode: 0 = choose by tile count, 1 or 4 = force (tuning / tests; same result) */
  float* normal_out;            /* optional (rows,W,3) dense: unit normal of the hit, 0 where nothing is hit */
  float* pos_out;               /* optional (rows,W,3) dense: hit point, 0 where nothing is hit */
  int64_t image_row_stride;     /* elements between consecutive output rows; 0 = dense (3*W, W, W). */
  int64_t depth_row_stride;     /* Lets image and depth rows interleave in one (rows, 4*W) slab so that a */
  int64_t nearest_row_stride;   /* multi-GPU frame is collected by a single gather. */
  void* ev_start;               /* optional hipEvent_t pair recorded on `stream` immediately before and */
  void* ev_stop;                /* after the frame's dominant kernel (measurement hook); NULL = off */
  const void* visibility;       /* srh_render_bwd, SRH_SHADING_TORCH: the (rows,W) uint64 light-visibility bits that
                                   srh_shadow_shade wrote for this frame, or NULL (no shadows) */
  const int32_t* view_row0;     /* srh_render_views only: HOST array of n_views first rows; view v renders rows
                                   [view_row0[v], view_row0[v] + row1 - row0).  NULL = every view renders [row0, row1) */
  int32_t stages;               /* srh_render_fwd, binned mode: 0 = the whole frame; SRH_STAGE_BIN = only the per-frame
                                   records and tile bins (into the workspace); SRH_STAGE_RENDER = only the render kernel,
                                   from the bins a SRH_STAGE_BIN call with the same arguments left in the workspace --
                                   the bin lists and the primitive records.
                                   Lets a caller run the latency-bound binning of frame i+1 on one stream beside the
                                   render kernel of frame i on another (surf_renderer_amd/pipeline.py) */
  int32_t counters_clean;       /* binned frames: 1 = the caller KNOWS that this workspace's bin counters are zero, so the
                                   frame needs no clearing launch: the workspace's last use was a binned frame of the SAME
                                   (objects, width, height) whose render stage ran without SRH_STAGE_KEEP_BINS (the render
                                   kernel leaves every counter it read at zero), and nothing else wrote to it since.
                                   0 = unknown (a fresh or re-purposed workspace): the library clears them first.  Wrong
                                   claims cannot make the kernels leave the workspace (every list access is bounded by
                                   the list's capacity) but give a wrong image. */
  int32_t per_view;             /* srh_render_views only: SRH_VIEWS_* bits -- which of `objects`, `lights`, `materials` point
                                   to ARRAYS of n_views structs (one scene per view) instead of one struct for all views.
                                   Every view's objects must have the same batches (types and counts) as view 0's. */
  int32_t reserved1;
} SrhParams;

/* SrhParams.per_view: the reference's real batch loop changes geometry, eye and light per element
 * (diffrend/torch/GAN/gan.py:325-378: disk.pos / disk.normal = samples[idx], camera eye, lights.pos[0]) */
enum { SRH_VIEWS_OBJECTS = 1, SRH_VIEWS_LIGHTS = 2, SRH_VIEWS_MATERIALS = 4 };

/* SrhParams.stages.  SRH_STAGE_KEEP_BINS (with SRH_STAGE_RENDER): the render kernel leaves the bin counters as they are,
 * so the same bins can be rendered again (measurement builds); the workspace is then NOT clean afterwards. */
enum { SRH_STAGE_BIN = 1, SRH_STAGE_RENDER = 2, SRH_STAGE_KEEP_BINS = 4 };

int srh_abi_version(void);
const char* srh_last_error(void);

/* bytes of caller-provided device scratch needed to render `objects` at up to width x height pixels
 * (per-frame primitive records and tile bins).  Returns 0 and sets srh_last_error on invalid input.
 * The buffer must be 256-byte aligned. */
size_t srh_workspace_bytes(const SrhObjects* objects, int32_t width, int32_t height);

/* replaces generate_rays (numpy/renderer.py:145-169): unit ray directions for rows [row0,row1),
 * written as the reference returns them, ray_dir (4, n) row-major with n = (row1-row0)*W. */
int srh_generate_rays(const SrhCamera* camera, int32_t row0, int32_t row1, float* ray_dir, void* stream);

/* replaces render() (numpy/renderer.py:204-272): rays -> all-pairs intersection -> nearest valid hit ->
 * Lambert shading over the point lights -> clip -> tonemap.
 *   image   (rows, W, 3) float32
 *   depth   (rows, W)    float32, +inf where nothing is hit (:228)
 *   nearest (rows, W)    int32 global primitive index, 0 where nothing is hit (:223); may be NULL */
int srh_render_fwd(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                   const SrhMaterials* materials, const SrhParams* params,
                   void* workspace, size_t workspace_bytes,
                   float* image, float* depth, int32_t* nearest, void* stream);

/* Gradient accumulators (device pointers; NULL = gradient not wanted).  srh_render_bwd ADDS into them with fp32
 * atomics, so the caller zero-fills them first; sums over many pixels are therefore reproducible only to
 * rounding.  Layouts equal the corresponding inputs. */
typedef struct SrhGrads {
  float* pos[SRH_MAX_SEGMENTS];      /* (count,4)   disk, plane, sphere; w gets no gradient */
  float* normal[SRH_MAX_SEGMENTS];   /* (count,4)   disk, plane, triangle (the un-normalised input normal) */
  float* radius[SRH_MAX_SEGMENTS];   /* (count)     sphere; a disc's radius has no gradient (masks are piecewise constant) */
  float* face[SRH_MAX_SEGMENTS];     /* (count,3,4) triangle: only vertex 0, the plane point, is differentiated */
  float* lights_pos;                 /* (n_lights,4) */
  float* colors;                     /* (n_colors,3) */
  float* albedo;                     /* (n_materials,3) */
  float* coeffs;                     /* (n_materials,3) SRH_SHADING_TORCH only: material coefficients (c0, c1, c2) */
  float* attenuation;                /* (n_lights,3)    SRH_SHADING_TORCH only: (kc, kl, kq) */
  float* ambient;                    /* (3)             SRH_SHADING_TORCH only */
} SrhGrads;

/* Analytic backward of srh_render_fwd: the vector-Jacobian product of (image, depth) w.r.t. the scene arrays for the
 * upstream gradients grad_image (rows,W,3) and grad_depth (rows,W; may be NULL), using the winners saved by the
 * forward pass (`nearest`, and `depth` to tell hit pixels from background).  Defined exactly as autograd through
 * the reference's differentiable backend defines it (diffrend/torch/renderer.py:136-355, torch/utils.py:238-366):
 * the nearest-hit selection and all masks are piecewise constant, so gradients flow only through the winner's hit
 * distance, hit point, normal, albedo and the lights.  With SRH_SHADING_TORCH the shading model differentiated is that
 * backend's Phong model (attenuation, specular coefficients, ambient; relus, the double_sided sign and the masks are
 * constants), and coeffs / attenuation / ambient gradients are available.  Row strides and the row range come from
 * `params` as in the forward call. */
int srh_render_bwd(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                   const SrhMaterials* materials, const SrhParams* params,
                   void* workspace, size_t workspace_bytes,
                   const float* grad_image, const float* grad_depth,
                   const int32_t* nearest, const float* depth,
                   const SrhGrads* grads, void* stream);

/* srh_render_bwd with the upstream gradients of the forward's extra outputs as well (SRH_SHADING_TORCH):
 * grad_normal and grad_pos (rows,W,3), dense like SrhParams.normal_out / pos_out, are d loss / d normal and
 * d loss / d pos, where normal is the hit's unit normal n^ = n / sqrt(|n|^2 + 3e-10) before the double_sided flip
 * (sphere: (p - c) likewise) and pos = origin + t d the hit point (per-pixel origin for orthographic cameras).  Any
 * of grad_image, grad_depth, grad_normal and grad_pos may be NULL, but not all four.  Without grad_image the kernel
 * differentiates the geometry alone (no light loops): light, colour and material gradients stay untouched.
 * Difference from the reference by design: at pixels that hit nothing, the upstream gradients of normal and pos are
 * ignored, as those of image and depth are (the reference gathers object 0's intersection there and differentiates
 * it).  With SRH_SHADING_NUMPY grad_normal / grad_pos must be NULL (that backend has no such outputs) and grad_image
 * is required.  Everything else is as for srh_render_bwd. */
int srh_render_bwd_aux(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                       const SrhMaterials* materials, const SrhParams* params,
                       void* workspace, size_t workspace_bytes,
                       const float* grad_image, const float* grad_depth,
                       const float* grad_normal, const float* grad_pos,
                       const int32_t* nearest, const float* depth,
                       const SrhGrads* grads, void* stream);

/* Camera gradients (device pointers to 4 floats each; NULL = not wanted).  srh_render_bwd_camera OVERWRITES them (it
 * does not add); w is written as 0. */
typedef struct SrhCameraGrads {
  float* eye;
  float* at;
  float* up;
} SrhCameraGrads;

/* srh_render_bwd_aux plus the gradients of the camera's eye, at and up (SRH_SHADING_TORCH only; SRH_SHADING_NUMPY is
 * refused with SRH_E_TYPE).  Defined as autograd through the reference's ray generation (torch/utils.py:402-427,
 * 439-478, its in-place division read as d = v / |v|) on top of the winners' hit distance, hit point, normal and view
 * direction; misses contribute nothing; fovy and focal_length have no gradient.  Every hit pixel's contribution is
 * reduced in fp64 over its workgroup and stored (no atomics) to `camera_scratch`, srh_camera_grad_scratch_bytes(W,
 * row1 - row0) bytes of caller-provided device memory (8-byte aligned; its previous contents do not matter: workgroups
 * without a hit store zeros); a one-workgroup kernel then adds the partial sums in a fixed order and applies the chain
 * rule of the look-at basis, so the three gradients are identical from run to run.  One launch more than
 * srh_render_bwd_aux.  A row slab sums over its own rows.  With all three camera pointers NULL the call is
 * srh_render_bwd_aux (the scratch is not looked at).  Added without an ABI version change: no existing struct or
 * signature changed. */
size_t srh_camera_grad_scratch_bytes(int32_t width, int32_t rows);
int srh_render_bwd_camera(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                          const SrhMaterials* materials, const SrhParams* params,
                          void* workspace, size_t workspace_bytes,
                          const float* grad_image, const float* grad_depth,
                          const float* grad_normal, const float* grad_pos,
                          const int32_t* nearest, const float* depth,
                          const SrhGrads* grads, const SrhCameraGrads* camera_grads,
                          void* camera_scratch, size_t camera_scratch_size, void* stream);

/* Many views in one call: the batch axis of the reference's real callers, which render one view per
 * render() call in a Python loop (diffrend/torch/GAN/gan.py:325-378, torch/batch_render.py:36-53).  `cameras` is an
 * array of n_views cameras with one viewport size; objects / lights / materials are one scene for all views or, per
 * SrhParams.per_view, one per view (same batch structure); `params` is shared (binned mode; row range and output row strides as
 * in srh_render_fwd, so a multi-GPU rank can render its slab of a whole batch of frames); the outputs are stacked:
 * view v starts v * rows * row_stride elements after view 0 in images (n_views,rows,W,3), depths (n_views,rows,W)
 * and nearests (may be NULL).  Every kernel of the
 * frame pipeline is launched once for the whole batch (the view is a grid dimension), so small views cost neither
 * three launches each nor an idle GPU.  Results equal srh_render_fwd per view.  The workspace must hold
 * srh_workspace_bytes_views(...) bytes.  Calls on one device are serialised on that device's staging ring. */
size_t srh_workspace_bytes_views(const SrhObjects* objects, int32_t width, int32_t height, int32_t n_views);
int srh_render_views(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                     const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                     float* images, float* depths, int32_t* nearests, void* stream);

/* srh_render_views with the torch backend's extra outputs for every view (SRH_SHADING_TORCH): `normals` and `poses` are
 * caller-owned, stacked and dense, (n_views,rows,W,3) float32 -- view v starts v * rows * W * 3 elements after view 0,
 * whatever the image row stride -- and are WRITTEN at every pixel of the rows rendered: the hit's unit normal (before
 * the double_sided flip) and the hit point, 0 where nothing is hit, equal to srh_render_fwd with SrhParams.normal_out /
 * pos_out per view.  Either may be NULL; with both NULL the call is srh_render_views.  With one of them set,
 * SRH_SHADING_NUMPY is refused with SRH_E_TYPE (that backend has no such outputs).  params->normal_out / pos_out stay
 * refused: they name one frame's buffers.  Perspective batches and orthographic ones (one frame per view) alike.
 * Everything else -- workspace, staging ring, checks -- is srh_render_views'.  Added without an ABI version change: no
 * existing struct or signature changed. */
int srh_render_views_aux(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                         const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                         float* images, float* depths, int32_t* nearests, float* normals, float* poses, void* stream);

/* The backward of a batch of views in one call: srh_render_bwd for every view of an srh_render_views batch, with
 * the view as a grid dimension of ONE backward launch (and of the record launches in front of it).  cameras, objects,
 * lights, materials and params are exactly what srh_render_views takes, with the same checks (per_view, row0 / row1,
 * view_row0, the row strides, one viewport size and one projection per call, 1..256 views); params->mode is ignored (a
 * backward bins nothing, so the forward may have run in any mode or one frame at a time), normal_out / pos_out and the
 * event hooks are refused.  Orthographic views (SRH_SHADING_TORCH) take the same kernel.
 *   grad_images, grad_depths   upstream gradients, stacked like the forward's outputs; grad_images is required (a
 *                              caller with a depth-only loss passes zeros), grad_depths may be NULL
 *   nearests, depths           the forward's stacked outputs
 *   params->visibility         SRH_SHADING_TORCH: the stacked (n_views,rows,W) uint64 bits of the views' shadow passes,
 *                              or NULL
 *   grads                      HOST array of n_views structs: where view v's gradients are ADDED.  A leaf all views share
 *                              has the same pointer in every struct (the fp32 atomics then sum over the views); a leaf a
 *                              view overrides points into that view's own buffer; NULL = not wanted.  The caller
 *                              zero-fills the buffers, as for srh_render_bwd.
 * The gradients equal srh_render_bwd per view, shared leaves summed.  No camera gradients and no normal / pos
 * gradients here: srh_render_views_bwd_camera below has both.  The workspace holds srh_workspace_bytes_views(...) bytes; only the
 * header and the views' primitive records are written -- bin counters and lists are not touched, so a workspace whose
 * counters were clean before the call (SrhParams.counters_clean) is clean after it.  The descriptors go through the
 * same per-device staging ring as srh_render_views, with the same consequences: the stream's device must be current
 * and the call cannot be stream-captured.  Added without an ABI version change: no existing struct or signature
 * changed. */
int srh_render_views_bwd(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                         const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                         const float* grad_images, const float* grad_depths, const int32_t* nearests,
                         const float* depths, const SrhGrads* grads, void* stream);

/* srh_render_views_bwd with the upstream gradients of the normal / pos outputs and with camera gradients for every view
 * (SRH_SHADING_TORCH only; SRH_SHADING_NUMPY is refused with SRH_E_TYPE): srh_render_bwd_camera for every view of a
 * batch, in the record launches, ONE backward launch and, when a view wants a camera gradient, ONE finish launch (one
 * workgroup per view).  cameras .. workspace_bytes, nearests, depths and params->visibility are srh_render_views_bwd's.
 *   grad_images, grad_depths   stacked like the forward's outputs (params' row strides)
 *   grad_normals, grad_poses   stacked dense (n_views,rows,W,3), like srh_render_views_aux's outputs
 *                              Any of the four may be NULL, but not all.  Without grad_images the geometry-only kernel
 *                              runs: light, colour and material gradients stay untouched, as in srh_render_bwd_aux.
 *                              At pixels that hit nothing all four are ignored.
 *   grads                      HOST array of n_views SrhGrads: ADDED into with fp32 atomics, exactly as in
 *                              srh_render_views_bwd (shared leaves share pointers; the caller zero-fills)
 *   camera_grads               HOST array of n_views SrhCameraGrads (device pointers to 4 floats each), or NULL when no
 *                              view wants any.  OVERWRITTEN, not added to: view v's eye / at / up gradients, w = 0;
 *                              a NULL member is not wanted, a view with three NULL members is skipped by the finish.
 *                              A view that hits nothing gets zeros.  When at least one member of one view is set, the
 *                              whole batch runs the camera variant of the kernel.
 *   camera_scratch             caller-owned device memory, srh_camera_grad_scratch_bytes_views(W, row1 - row0, n_views)
 *                              bytes, 8-byte aligned: a 256-byte aligned head that receives the views' finish
 *                              descriptors (written by a copy on the stream) and one srh_camera_grad_scratch_bytes
 *                              slice of fp64 workgroup partial sums per view.  Its previous contents do not matter
 *                              (workgroups without a hit store zeros).  Size and alignment are checked
 *                              (SRH_E_WORKSPACE, the needed size in the message) only when a camera gradient is wanted;
 *                              otherwise it is not looked at and may be NULL.  It must stay untouched until the call's
 *                              work on the stream has finished.
 * srh_camera_grad_scratch_bytes_views returns 0 and sets srh_last_error for width < 1, rows < 1 or n_views outside
 * 1..256.  The camera gradients use no atomics and fixed-order fp64 sums (k_camera_finish's, per view): identical from
 * run to run, and equal to srh_render_bwd_camera per view.  The workspace is srh_workspace_bytes_views(...) bytes and is
 * written as srh_render_views_bwd writes it (header and records, never the bin counters).  Staging ring, current device
 * and "cannot be stream-captured" as for srh_render_views_bwd.  Added without an ABI version change: no existing struct
 * or signature changed. */
size_t srh_camera_grad_scratch_bytes_views(int32_t width, int32_t rows, int32_t n_views);
int srh_render_views_bwd_camera(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects,
                                const SrhLights* lights, const SrhMaterials* materials, const SrhParams* params,
                                void* workspace, size_t workspace_bytes,
                                const float* grad_images, const float* grad_depths,
                                const float* grad_normals, const float* grad_poses,
                                const int32_t* nearests, const float* depths,
                                const SrhGrads* grads, const SrhCameraGrads* camera_grads,
                                void* camera_scratch, size_t camera_scratch_size, void* stream);

/* The torch backend's `shadow=True` (diffrend/torch/renderer.py:291-314) as a second pass over a frame rendered by
 * srh_render_fwd with the same camera / scene / params (SRH_SHADING_TORCH): per hit pixel and light a shadow ray from
 * the fragment (started 0.1 towards the light) against every primitive, all pairs in fp64; a light is visible unless
 * a primitive other than the fragment's own is hit before it.  `image` (rows,W,3) is overwritten with the re-shaded
 * frame; `visibility` (rows,W) uint64, bit l = light l visible, may be NULL.
 * With a workspace of srh_shadow_workspace_bytes(...) bytes the candidates of a shadow ray come from tile bins built
 * in each light's own screen space (every candidate still goes through the same fp64 test, so the result equals the
 * all-pairs pass bit for bit); with the smaller srh_workspace_bytes(...) workspace, or params->mode =
 * SRH_MODE_EXACT, the pass is the reference's O(pixels x lights x primitives) loop. */
size_t srh_shadow_workspace_bytes(const SrhObjects* objects, int32_t width, int32_t height, int32_t n_lights);
int srh_shadow_shade(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                     const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                     const int32_t* nearest, const float* depth, float* image, uint64_t* visibility, void* stream);

/* Measurement helper: where a binned frame's list lengths live in its workspace, so that a caller can count the
 * (pixel, primitive) tests a frame really executes (bench.py: executed_pair_tests) or weigh image rows by their work
 * (surf_renderer_amd.dist.cost_weighted_slabs).  After an SRH_STAGE_BIN call for rows [row0, row1), the 32-bit words
 * at workspace + *offset_bytes hold:  [4 * set + s] length of batch s's frame-wide list, with set = word [9];
 * [64 + s * *ntiles_pad + ty * *tiles_x + tx] length of the bin of batch s and tile (tx, ty) -- lists longer than
 * *bin_cap are cut there (their primitives are on the frame-wide list instead).  The render stage zeroes them again. */
int srh_bin_counters(const SrhObjects* objects, int32_t width, int32_t height, int32_t row0, int32_t row1,
                     size_t* offset_bytes, int32_t* tiles_x, int32_t* tiles_y, int32_t* ntiles_pad, int32_t* bin_cap);

/* What the host has proved about a camera's primary rays, as the render entry points decide it for every frame
 * (`orthonormal`: the basis of SRH_SHADING_TORCH).  *flags bit 0: the three divisions by |D| may share one reciprocal;
 * bit 1 (only with bit 0): |D|^2 is bounded over the frame and the binned finish rounds take its square root without
 * range guards.  Both are bit-identical to the plain forms; 0 for a camera of extreme or non-finite magnitudes.  With
 * SRH_ROOT_GUARDS set in the environment bit 1 is never set (tests compare the two forms on one camera). */
int srh_camera_ray_flags(const SrhCamera* camera, int32_t orthonormal, int32_t* flags);

/* measurement helpers: timing-enabled HIP events usable as SrhParams.ev_start / ev_stop.
 * srh_event_elapsed_ms waits for `stop` to complete (the only call here that blocks the host). */
int srh_event_create(void** event);
int srh_event_destroy(void* event);
int srh_event_elapsed_ms(void* start, void* stop, float* ms);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's splat renderer, render_splats_along_ray (diffrend/torch/renderer.py:537-751): one splat per pixel of a
 * W x H grid, given by its camera-space depth z, shaded in camera coordinates with the torch backend's Phong model
 * (double_sided off, no tonemap, relu over the light sum).  Normals are given or estimated by the reference's plane fit
 * over the reflected 3x3 stencil; samples K > 1 shades K x K sub-rays per splat on the splat's plane.  Many views per
 * call: z, normals, light_vis, the eye and the light positions may differ per view (the GAN's batch), everything else is
 * shared.  These entry points were added without an ABI version change: no existing struct or signature changed.
 * Conventions as above: caller-owned device buffers, enqueue only, no synchronisation or allocation, argument checks
 * before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhSplatParams {
  int32_t n_views;              /* B >= 1 */
  int32_t width, height;        /* base grid W x H (camera viewport); >= 2 each when normals are estimated */
  int32_t samples;              /* K in 1..8: outputs are (B, K H, K W, ...) */
  int32_t pos_cols;             /* 1: pos holds z (N); 3: pos is (N,3) and only column 2 (z) is read */
  int32_t use_quartic;          /* attenuation uses d^4 instead of d^2 */
  int32_t shade;                /* 1: shade the image; 0: geometry only (depth, pos, normal; norm_depth_image_only) */
  int32_t reserved;
  double fovy, focal_length;    /* radians; f > 0 */
  double at[3], up[3];          /* camera.at / camera.up (shared by all views; w dropped as the reference does) */
} SrhSplatParams;

/* Device inputs; N = W * H.  A view stride of 0 shares the array between all views. */
typedef struct SrhSplatInputs {
  const float* pos;             /* (B, N, pos_cols) with pos_view_stride elements between views */
  int64_t pos_view_stride;
  const float* normal;          /* (N,3) per view, used as given; NULL: estimate (plane fit) */
  int64_t normal_view_stride;
  const float* light_vis;       /* (n_lights, N) per view, multiplies colour x albedo; NULL: all lights visible */
  int64_t light_vis_view_stride;
  const float* eye;             /* (3) per view: camera.eye[:3] */
  int64_t eye_view_stride;
  int64_t lights_pos_view_stride; /* SrhLights.pos is (n_lights,4) per view with this stride */
  const int32_t* material_idx;  /* (N) shared; NULL: material 0 everywhere */
} SrhSplatInputs;

/* Gradients.  pos, normal and light_vis are WRITTEN (dense per view, no atomics: identical from run to run):
 * pos (B, N, pos_cols) with zeros outside column pos_cols - 1, normal (B, N, 3) (given normals only), light_vis
 * (B, n_lights, N).  The scene parameters are ADDED with fp32 atomics (zero-fill them first) in their input layouts:
 * lights_pos (n_lights,4) per view at lights_pos_view_stride, colors, attenuation, ambient, albedo, coeffs.
 * NULL = not wanted.  The camera's gradient is srh_splat_bwd_view's.  A geometry-only frame (shade = 0) depends on none of light_vis,
 * the lights, colours and materials: srh_splat_bwd refuses those gradient buffers then (SRH_E_TYPE). */
typedef struct SrhSplatGrads {
  float* pos;
  float* normal;
  float* light_vis;
  float* lights_pos;
  float* colors;
  float* attenuation;
  float* ambient;
  float* albedo;
  float* coeffs;
} SrhSplatGrads;

/* bytes of device scratch srh_splat_bwd needs (8-byte aligned; 0 for given normals); 0 and srh_last_error on bad input */
size_t srh_splat_workspace_bytes(const SrhSplatParams* params, const SrhSplatInputs* inputs);

/* image (B,KH,KW,3) (may be NULL when params->shade == 0), depth (B,KH,KW), pos (B,KH,KW,3), normal (B,KH,KW,3).
 * lights / materials as for SRH_SHADING_TORCH (attenuation, ambient and coeffs optional). */
int srh_splat_fwd(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                  const SrhMaterials* materials, float* image, float* depth, float* pos, float* normal, void* stream);

/* Vector-Jacobian product of srh_splat_fwd for the upstream gradients of its four outputs (same layouts; any may be
 * NULL, grad_image must be NULL when shade = 0).  Relus and the z >= 0 clamp are constants (no gradient through them); at a point at the origin the depth
 * has no gradient. */
int srh_splat_bwd(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                  const SrhMaterials* materials, void* workspace, size_t workspace_bytes,
                  const float* grad_image, const float* grad_depth, const float* grad_pos, const float* grad_normal,
                  const SrhSplatGrads* grads, void* stream);

/* srh_splat_bwd plus the camera's gradient up to the per-view matrix: the camera enters only through the lights'
 * camera coordinates L = M (l_xyz, l_w), M the view's 3 x 4 world-to-camera matrix as the kernels build it from eye /
 * at / up, and grad_view (B, 12) fp64, row-major per view, is d loss / d M = sum over pixels, sub-pixels and lights of
 * g_L (x) (l_x, l_y, l_z, l_w), WRITTEN with every element once (the chain from the matrix to eye / at / up is the
 * caller's).  The buffers of `grads` may then all be NULL; a geometry-only frame (shade = 0) does not depend on the
 * camera and is refused (SRH_E_TYPE).  view_workspace: srh_view_grad_workspace_bytes(n_views, width, height) bytes of
 * the BASE grid, 8-byte aligned; the partial sums are added without atomics in an order that depends only on width x
 * height, so grad_view is identical from run to run and a view of a batch gets the bits of the same view alone.  The
 * gradients of `grads` are srh_splat_bwd's.  Added without an ABI version change. */
int srh_splat_bwd_view(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                       const SrhMaterials* materials, void* workspace, size_t workspace_bytes, const float* grad_image,
                       const float* grad_depth, const float* grad_pos, const float* grad_normal,
                       const SrhSplatGrads* grads, double* grad_view, void* view_workspace,
                       size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's NDC splat renderer, render_splats_NDC (diffrend/torch/renderer.py:358-474): one splat per pixel of a
 * W x H grid, given by its position in normalised device coordinates and a normal.  With m00 = 1 / (aspect tan(fovy/2)),
 * m11 = 1 / tan(fovy/2), m22 = (near + far) / (far - near), m23 = -2 near far / (far - near), aspect = W / H:
 *   q = (x / m00, y / m11, -w, (z - m22 w) / m23),  P = q.xyz / q.w,  depth = |P|
 * (w = 1 for three-column positions).  The normal is used as given, neither transformed nor normalised.  Shading is the
 * torch backend's Phong in camera coordinates with the view direction -P NOT normalised, double_sided honoured (the sign
 * of view . normal multiplies the diffuse and the specular dot before their relus), the ambient term once per light, a
 * relu over the light sum, no near / far mask and no tonemap.  Many views per call: positions, normals, the eye and the
 * light positions may differ per view, everything else is shared.  These entry points were added without an ABI version
 * change: no existing struct or signature changed.  Conventions as above: caller-owned device buffers, enqueue only, no
 * synchronisation or allocation, argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhSplatNdcParams {
  int32_t n_views;              /* B >= 1 */
  int32_t width, height;        /* the grid W x H (camera viewport); N = W * H splats per view, row-major */
  int32_t pos_cols;             /* 3: pos is (N,3), w = 1; 4: pos is (N,4) */
  int32_t use_quartic;          /* attenuation uses d^4 instead of d^2 */
  int32_t double_sided;         /* flip the shading to the side of the normal the camera is on */
  int32_t shade;                /* 1: shade the image; 0: geometry only (depth, pos; norm_depth_image_only) */
  int32_t reserved;
  double fovy;                  /* radians, in (0, pi) */
  double near_clip, far_clip;   /* 0 < near < far */
  double at[3], up[3];          /* camera.at / camera.up (shared by all views; w dropped as the reference does) */
} SrhSplatNdcParams;

/* Device inputs.  A view stride of 0 shares the array between all views. */
typedef struct SrhSplatNdcInputs {
  const float* pos;             /* (B, N, pos_cols) with pos_view_stride elements between views */
  int64_t pos_view_stride;
  const float* normal;          /* (N,3) per view, used as given; read only when shade = 1 (may be NULL otherwise) */
  int64_t normal_view_stride;
  const float* eye;             /* (3) per view: camera.eye[:3] */
  int64_t eye_view_stride;
  int64_t lights_pos_view_stride; /* SrhLights.pos is (n_lights,4) per view with this stride */
  const int32_t* material_idx;  /* (N) shared; NULL: material 0 everywhere */
} SrhSplatNdcInputs;

/* Gradients.  pos (B, N, pos_cols: every column) and normal (B, N, 3) are WRITTEN, each element by the lane that owns
 * the splat (no atomics, no zero-fill, no workspace: identical from run to run).  The scene parameters are ADDED with
 * fp32 atomics (zero-fill them first) in their input layouts, as SrhSplatGrads: lights_pos (n_lights,4) per view at
 * lights_pos_view_stride, colors, attenuation, ambient, albedo, coeffs.  NULL = not wanted.  The camera's
 * gradient is srh_splat_ndc_bwd_view's.  A geometry-only frame (shade = 0) depends on none of the lights, colours and materials:
 * srh_splat_ndc_bwd refuses those gradient buffers then (SRH_E_TYPE). */
typedef struct SrhSplatNdcGrads {
  float* pos;
  float* normal;
  float* lights_pos;
  float* colors;
  float* attenuation;
  float* ambient;
  float* albedo;
  float* coeffs;
} SrhSplatNdcGrads;

/* image (B,H,W,3) (may be NULL when params->shade == 0), depth (B,H,W), pos (B,H,W,3): every element is written.
 * lights / materials as for srh_splat_fwd (attenuation, ambient and coeffs optional), n_lights in 1..SRH_MAX_LIGHTS. */
int srh_splat_ndc_fwd(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                      const SrhMaterials* materials, float* image, float* depth, float* pos, void* stream);

/* Vector-Jacobian product of srh_splat_ndc_fwd for the upstream gradients of its three outputs (same layouts; any may
 * be NULL, not all; grad_image must be NULL when shade = 0).  Relus and the sign of double_sided are constants (no
 * gradient through them); at a point at the origin the depth has no gradient. */
int srh_splat_ndc_bwd(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                      const SrhMaterials* materials, const float* grad_image, const float* grad_depth,
                      const float* grad_pos, const SrhSplatNdcGrads* grads, void* stream);

/* srh_splat_ndc_bwd plus grad_view (B, 12) fp64, the gradient with respect to the view's 3 x 4 world-to-camera matrix
 * through the lights' camera coordinates, exactly as srh_splat_bwd_view: every element WRITTEN once (zeros without
 * grad_image), no atomics, the buffers of `grads` may all be NULL, shade = 0 is refused (SRH_E_TYPE), view_workspace of
 * srh_view_grad_workspace_bytes(n_views, width, height) bytes, 8-byte aligned.  Added without an ABI version change. */
int srh_splat_ndc_bwd_view(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                           const SrhMaterials* materials, const float* grad_image, const float* grad_depth,
                           const float* grad_pos, const SrhSplatNdcGrads* grads, double* grad_view,
                           void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The geometric regularisers the reference's trainers put on every rendered splat view (diffrend/torch/GAN/gan.py:
 * 601-640 with diffrend/torch/utils.py:731-851), for B views per call.  Inputs are what srh_splat_fwd writes: pos,
 * normal, image (B, H, W, 3) and depth (B, H, W), dense, with H x W the OUTPUT grid (K H x K W at samples = K).
 * d_k(x) = x[neighbour k] - x[centre] over the 3 x 3 stencil without its centre, reflected at the borders; N = H W.
 * Terms, in this order (SRH_REG_TERMS of them per view):
 *   0 z                        mean (s relu(z_min - |p_z|))^2 + (s relu(|p_z| - z_max))^2,  s = z_scale
 *   1 unit_normal              mean (c (|n| - 1))^2,  c = unit_normal_scale
 *   2 normal_consistency       mean over the 8 N pairs of |u_k . n|,  u_k = d_k(pos) / sqrt(|d_k|^2 + 3e-10)
 *   3 spatial                  mean over the 8 N pairs of sum_c |d_k(pos)_c|
 *   4 spatial_var              1 / (var p_x + var p_y + var p_z + 1e-4), unbiased variances over the N pixels
 *   5 image_depth_consistency  mean over the 8 N pairs of | |d_k(mean_c image)| - |d_k(depth)| |
 *   6 away_from_camera         SUM over the pixels of relu(n . p / sqrt(|p|^2 + 3e-10))
 * fp64 arithmetic, fp32 results, no atomics: values and gradients are identical from run to run.  Gradients follow
 * autograd's conventions (|.| and relu have gradient 0 at 0) except that a normal that is exactly zero gets no
 * unit_normal gradient (autograd: NaN).  These entry points were added without an ABI version change.  Conventions as
 * above: caller-owned device buffers, enqueue only, no synchronisation or allocation, argument checks before any HIP
 * call.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_REG_TERMS 7
#define SRH_REG_STATS 4           /* doubles per view: mean p_x, p_y, p_z and the variance sum */

typedef struct SrhRegularizerParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 2 each (reflection), W H <= 2^24 */
  int32_t reserved;
  double z_min, z_max;          /* z_min <= z_max */
  double z_scale;               /* s */
  double unit_normal_scale;     /* c */
} SrhRegularizerParams;

/* bytes of device scratch srh_regularizers_fwd needs (8-byte aligned): one row of partial sums per workgroup; 0 and
 * srh_last_error on bad input */
size_t srh_regularizers_workspace_bytes(int32_t n_views, int32_t width, int32_t height);

/* terms (B, SRH_REG_TERMS) fp32; stats (B, SRH_REG_STATS) fp64, which srh_regularizers_bwd reads */
int srh_regularizers_fwd(const SrhRegularizerParams* params, const float* pos, const float* normal, const float* image,
                         const float* depth, void* workspace, size_t workspace_bytes, float* terms, double* stats,
                         void* stream);

/* Vector-Jacobian product for grad_terms (B, SRH_REG_TERMS) fp32 and the stats of the forward call on the same inputs.
 * g_pos, g_normal, g_image (B, H, W, 3) and g_depth (B, H, W) are WRITTEN, every element once (no zero-fill needed);
 * any may be NULL = not wanted, not all. */
int srh_regularizers_bwd(const SrhRegularizerParams* params, const float* pos, const float* normal, const float* image,
                         const float* depth, const double* stats, const float* grad_terms, float* g_pos,
                         float* g_normal, float* g_image, float* g_depth, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's surfel re-projection layer, projection_renderer_differentiable_fast (diffrend/torch/
 * projection_layer.py:170-278), for B views per call: N = W H surfels per view (world position and a D-channel value)
 * are projected into the view's camera, spread bilinearly over four pixels with weighted-blended order-independent
 * transparency, blurred with a separable Gaussian and optionally merged with a second image through the soft coverage
 * mask.  Restated as gathers: no float atomic in either direction, fp64 arithmetic, fp32 results, values and gradients
 * identical from run to run.  The camera is not differentiable.
 *
 * One forward is three steps, because the ordering is the caller's:
 *   srh_projection_keys   writes one record per surfel into the workspace and keys (B, N) int32: the surfel's cell on
 *                         the (W + 1) x (H + 1) grid of cells that reach the frame, (W + 1)(H + 1) for a surfel that
 *                         does not
 *   the caller            makes order (B, N) int32: per view a STABLE ASCENDING permutation of that view's keys (ties in
 *                         ascending surfel index), which fixes the order of every sum
 *   srh_projection_fwd    the rest.
 * These entry points were added without an ABI version change.  Conventions as above: caller-owned device buffers,
 * enqueue only, no synchronisation or allocation, argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_PROJ_MAX_CHANNELS 4
#define SRH_PROJ_MAX_BLUR_HALF 64

#define SRH_PROJ_USE_DEPTH 1            /* weight by exp(-2 z) */
#define SRH_PROJ_USE_CENTER_DIST 2      /* weight by the Gaussian of the distance to the cell's pixel centre */
#define SRH_PROJ_BLUR_ROTATED 4         /* blur the rotated image before the merge */
#define SRH_PROJ_DETACH_MASK 8          /* the reference's detach_mask (wins over DETACH_MASK2, as there) */
#define SRH_PROJ_DETACH_MASK2 16
#define SRH_PROJ_DETACH_DEPTH_MERGE 32  /* no gradient through the depth, as a weight or as a blended value */

/* the three buffers srh_projection_workspace_bytes sizes */
#define SRH_PROJ_WS_FWD 0               /* scratch shared by srh_projection_keys and srh_projection_fwd */
#define SRH_PROJ_WS_SAVED 1             /* written by srh_projection_fwd, read by srh_projection_bwd */
#define SRH_PROJ_WS_BWD 2               /* scratch of srh_projection_bwd */

typedef struct SrhProjectionParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24; N = W H surfels per view */
  int32_t channels;             /* D in 1..SRH_PROJ_MAX_CHANNELS */
  int32_t flags;                /* SRH_PROJ_* bits */
  int32_t blur_half;            /* half-width of the blur in 0..SRH_PROJ_MAX_BLUR_HALF; 0 = no blur */
  double fovy, focal_length;    /* shared by the views: 0 < fovy < pi, focal_length > 0 */
  double taps[SRH_PROJ_MAX_BLUR_HALF + 1];   /* taps[|d|] for d in -blur_half..blur_half, finite; the caller normalises */
} SrhProjectionParams;

/* bytes of the buffer `which` (SRH_PROJ_WS_*; 8-byte aligned); 0 and srh_last_error on bad input */
size_t srh_projection_workspace_bytes(const SrhProjectionParams* params, int32_t which);

/* view (B, 12) fp64: each view's world-to-camera matrix, 3 rows of 4; surfels (B, N, 3) fp32; keys (B, N) int32 out */
int srh_projection_keys(const SrhProjectionParams* params, const double* view, const float* surfels, void* workspace,
                        size_t workspace_bytes, int32_t* keys, void* stream);

/* rgb (B, N, D) fp32; rotated the same or NULL = no merge; keys and workspace as srh_projection_keys left them; order:
 * per view a stable ascending permutation of the keys (an entry outside 0..N-1 is skipped).  saved (SRH_PROJ_WS_SAVED)
 * may be NULL when no backward will follow.  out, image1 (B, N, D) and mask (B, N) fp32 are written; depth (B, N) may
 * be NULL = not wanted. */
int srh_projection_fwd(const SrhProjectionParams* params, const float* rgb, const float* rotated, const int32_t* keys,
                       const int32_t* order, void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes,
                       float* out, float* mask, float* image1, float* depth, void* stream);

/* Vector-Jacobian product.  view, surfels, rgb and the flags as in the forward call that wrote `saved`; `rotated` is
 * only tested against NULL.  Upstream gradients g_out, g_image1 (B, N, D), g_mask, g_depth (B, N) fp32: NULL = none,
 * not all.  grad_surfels (B, N, 3), grad_rgb, grad_rotated (B, N, D) are WRITTEN, every element once; any may be NULL
 * = not wanted, not all; grad_rotated needs `rotated`. */
int srh_projection_bwd(const SrhProjectionParams* params, const double* view, const float* surfels, const float* rgb,
                       const float* rotated, const void* saved, size_t saved_bytes, void* workspace,
                       size_t workspace_bytes, const float* g_out, const float* g_mask, const float* g_image1,
                       const float* g_depth, float* grad_surfels, float* grad_rgb, float* grad_rotated, void* stream);

/* The camera gradient of the depth lift and of the two warps, up to the per-view matrix: each *_bwd_view entry point is
 * its layer's *_bwd plus grad_view (B, 12) fp64, the gradient with respect to the `view` table the layer was handed,
 * WRITTEN with every element once (the chain from the matrix to eye / at / up is the caller's).  The other grad_*
 * outputs may then all be NULL.  view_workspace: srh_view_grad_workspace_bytes bytes, 8-byte aligned, one set of
 * partial sums per workgroup; they are added without atomics in an order that depends only on width x height, so the
 * result is identical from run to run and a view of a batch gets the bits of the same view alone.  Added without an
 * ABI version change. */
size_t srh_view_grad_workspace_bytes(int32_t n_views, int32_t width, int32_t height);

int srh_projection_bwd_view(const SrhProjectionParams* params, const double* view, const float* surfels,
                            const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                            void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                            const float* g_image1, const float* g_depth, float* grad_surfels, float* grad_rgb,
                            float* grad_rotated, double* grad_view, void* view_workspace, size_t view_workspace_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's backward-warp ("pull") re-projection, projection_reverse_renderer (diffrend/torch/
 * projection_layer.py:281-333), for B views per call.  Each of the N = W H pixels of the target view has a surfel
 * (out_pos, world coordinates) that is projected into the source camera (camera 1), where the source image rgb is
 * sampled bilinearly (zero padding, texel centres at integers of pixel coordinate - 1/2); a pixel that leaves the frame
 * by the reference's 0.5-pixel test, or whose depth in camera 1 exceeds the twice-resampled depth of the source view's
 * own surfels (in_pos, seen by camera 2) by more than depth_epsilon, is masked out, and `rotated` fills the holes.
 * fp64 arithmetic, fp32 results, no float atomic in either direction, values and gradients identical from run to run.
 * The cameras are not differentiable.
 *
 * The forward is one call.  A backward that wants grad_rgb or grad_in_pos is three steps, because the ordering is the
 * caller's, as for srh_projection_*:
 *   srh_reverse_projection_keys   keys (B, N) int32: each pixel's sample cell on the (W + 1) x (H + 1) grid of cells
 *                                 that reach the frame, (W + 1)(H + 1) for a sample that does not; and one record per
 *                                 pixel at the head of the backward workspace
 *   the caller                    order (B, N) int32: per view a STABLE ASCENDING permutation of that view's keys
 *   srh_reverse_projection_bwd    the rest.
 * A backward that wants neither skips the first two and passes keys = order = workspace = NULL.  Added without an ABI
 * version change.  Conventions as above: caller-owned device buffers, enqueue only, no synchronisation or allocation,
 * argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_RPROJ_WS_FWD 0              /* scratch of srh_reverse_projection_fwd */
#define SRH_RPROJ_WS_BWD 1              /* shared by srh_reverse_projection_keys and srh_reverse_projection_bwd */

typedef struct SrhReverseProjectionParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24: the frame of rgb and of both cameras */
  int32_t channels;             /* D in 1..SRH_PROJ_MAX_CHANNELS */
  double fovy1, focal_length1;  /* camera 1, shared by the views: 0 < fovy < pi, focal_length > 0 */
  double fovy2, focal_length2;  /* camera 2 */
  double depth_epsilon;         /* finite */
} SrhReverseProjectionParams;

/* bytes of the buffer `which` (SRH_RPROJ_WS_*; 8-byte aligned); 0 and srh_last_error on bad input */
size_t srh_reverse_projection_workspace_bytes(const SrhReverseProjectionParams* params, int32_t which);

/* view1, view2 (B, 12) fp64: each view's world-to-camera matrices, 3 rows of 4; rgb (B, N, D), in_pos, out_pos (B, N, 3)
 * fp32; rotated (B, N, D) or NULL = no merge; keep (B, N) fp32 or NULL: a plane the mask is multiplied by (dropout).
 * mask (B, N) and image1 (B, N, D) are written; out (B, N, D) is written with `rotated` and not looked at without (the
 * result is then image1); depth (B, N) may be NULL = not wanted.  Nothing is kept for the backward. */
int srh_reverse_projection_fwd(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                               const float* rgb, const float* in_pos, const float* out_pos, const float* rotated,
                               const float* keep, void* workspace, size_t workspace_bytes, float* out, float* mask,
                               float* image1, float* depth, void* stream);

/* keys (B, N) int32 out; workspace: SRH_RPROJ_WS_BWD */
int srh_reverse_projection_keys(const SrhReverseProjectionParams* params, const double* view1, const float* out_pos,
                                void* workspace, size_t workspace_bytes, int32_t* keys, void* stream);

/* Vector-Jacobian product.  Inputs as in the forward call; mask as that call wrote it.  Upstream gradients g_out,
 * g_image1 (B, N, D), g_depth (B, N) fp32: NULL = none, not all; g_out is the gradient of the `out` of a call with a
 * rotated image (without one `out` is image1, and its gradient belongs in g_image1).  The mask carries no gradient.
 * grad_rgb, grad_rotated (B, N, D), grad_in_pos, grad_out_pos (B, N, 3) are WRITTEN, every element once; any may be
 * NULL = not wanted, not all.  grad_rgb and grad_in_pos need keys and workspace as srh_reverse_projection_keys left
 * them and `order` (an entry outside 0..N-1 is skipped); without either of the two, keys, order and workspace are not
 * looked at. */
int srh_reverse_projection_bwd(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                               const float* rgb, const float* in_pos, const float* out_pos, const float* mask,
                               const int32_t* keys, const int32_t* order, void* workspace, size_t workspace_bytes,
                               const float* g_out, const float* g_image1, const float* g_depth, float* grad_rgb,
                               float* grad_in_pos, float* grad_out_pos, float* grad_rotated, void* stream);

/* srh_reverse_projection_bwd plus the gradients of the two view tables (see srh_projection_bwd_view): grad_view1,
 * grad_view2 (B, 12) fp64, either may be NULL = not wanted, not both.  Camera 2 reaches the results through the values
 * of the new depth alone, so rows 0 and 1 of grad_view2 are exactly 0, and grad_view2 needs keys, order and workspace
 * like grad_in_pos. */
int srh_reverse_projection_bwd_view(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                                    const float* rgb, const float* in_pos, const float* out_pos, const float* mask,
                                    const int32_t* keys, const int32_t* order, void* workspace, size_t workspace_bytes,
                                    const float* g_out, const float* g_image1, const float* g_depth, float* grad_rgb,
                                    float* grad_in_pos, float* grad_out_pos, float* grad_rotated, double* grad_view1,
                                    double* grad_view2, void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's dense Gaussian re-projection, projection_renderer_differentiable (diffrend/torch/projection_layer.py:
 * 108-152), for B views per call: every one of the N = W H surfels of a view (world position and a D-channel value)
 * contributes to every one of its W H pixels (i, j) with the weight exp(-((u - i)^2 + (v - j)^2) / (2 sigma^2)), (u, v)
 * the surfel's pixel coordinate less 1/2 -- surfels outside the frame and behind the camera included.  mask = the sum
 * of the weights (not normalised), S = the weighted sum of the values;
 *   out = S / (mask + 1e-10)        without a rotated image
 *   out = S + rotated (1 - mask)    with one.
 * No buffer grows with W H x N: the weight is separable and is formed tile by tile.  fp64 arithmetic, fp32 results, no
 * atomic in either direction, every sum in a fixed order: values and gradients are identical from run to run and a
 * batch equals its views.  The camera is not differentiable.  Added without an ABI version change.  Conventions as
 * above: caller-owned device buffers, enqueue only, no synchronisation or allocation, argument checks before any HIP
 * call.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_DPROJ_WS_FWD 0              /* scratch of srh_dense_projection_fwd */
#define SRH_DPROJ_WS_SAVED 1            /* written by srh_dense_projection_fwd, read by srh_dense_projection_bwd */
#define SRH_DPROJ_WS_BWD 2              /* scratch of srh_dense_projection_bwd */
#define SRH_DPROJ_WS_VIEW 4             /* view_workspace of srh_dense_projection_bwd_view: B ceil(N / 64) 96 bytes
                                           (3 stays refused, as before this value existed) */

typedef struct SrhDenseProjectionParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24; N = W H surfels per view */
  int32_t channels;             /* D in 1..SRH_PROJ_MAX_CHANNELS */
  int32_t has_rotated;          /* 0: out = S / (mask + 1e-10); 1: out = S + rotated (1 - mask) */
  int32_t reserved;             /* 0 */
  double sigma;                 /* of the Gaussian, in pixels: positive and finite */
  double fovy, focal_length;    /* shared by the views: 0 < fovy < pi, focal_length > 0 */
} SrhDenseProjectionParams;

/* bytes of the buffer `which` (SRH_DPROJ_WS_*; 8-byte aligned), each linear in B W H; 0 and srh_last_error on bad
 * input */
size_t srh_dense_projection_workspace_bytes(const SrhDenseProjectionParams* params, int32_t which);

/* view (B, 12) fp64: each view's world-to-camera matrix, 3 rows of 4; surfels (B, N, 3), rgb (B, N, D) fp32; rotated
 * (B, N, D) fp32 with has_rotated, NULL without.  saved (SRH_DPROJ_WS_SAVED) may be NULL when no backward will follow.
 * out (B, N, D) and mask (B, N) fp32 are written, every element once. */
int srh_dense_projection_fwd(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                             const float* rgb, const float* rotated, void* workspace, size_t workspace_bytes,
                             void* saved, size_t saved_bytes, float* out, float* mask, void* stream);

/* Vector-Jacobian product.  Inputs as in the forward call that wrote `saved`.  Upstream gradients g_out (B, N, D) and
 * g_mask (B, N) fp32: NULL = none, not both.  grad_surfels (B, N, 3), grad_rgb, grad_rotated (B, N, D) are WRITTEN,
 * every element once; any may be NULL = not wanted, not all; grad_rotated needs has_rotated. */
int srh_dense_projection_bwd(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                             const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                             void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                             float* grad_surfels, float* grad_rgb, float* grad_rotated, void* stream);

/* srh_dense_projection_bwd plus the gradient of the view table (see srh_projection_bwd_view): grad_view (B, 12) fp64,
 * WRITTEN with every element once; grad_surfels, grad_rgb and grad_rotated may then all be NULL.  Every surfel
 * contributes, those outside the frame and behind the camera too.  view_workspace: SRH_DPROJ_WS_VIEW bytes, 8-byte
 * aligned -- this layer's surfel kernel runs one wave per workgroup, so the size is not srh_view_grad_workspace_bytes.
 * Without a camera gradient to form, call srh_dense_projection_bwd: it launches nothing more than before.  Added without
 * an ABI version change. */
int srh_dense_projection_bwd_view(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                                  const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                                  void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                                  float* grad_surfels, float* grad_rgb, float* grad_rotated, double* grad_view,
                                  void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The depth-map-to-surfels front end of the reference's re-projection loops (diffrend/torch/projection_layer.py:749-750:
 * cam_to_world_batched(z_to_pcl_CC_batched(-depth, camera), None, camera)['pos']), for B views per call.  Pixel
 * q = i W + j of a view with depth d = max(depth, 0) (positive in front of the camera) becomes
 *   P_cc = (d x_j / f, d y_i / f, -d),  x_j = fp32(linspace(-1, 1, W)_j w / 2),  y_i = fp32(linspace(1, -1, H)_i h / 2)
 * (numpy's linspace, the grid of srh_splat_fwd), and in the world frame P_wc = R P_cc + eye.  fp64 arithmetic, one fp32
 * store per element, no atomic, every element written once.  The camera is not differentiable.  Added without an ABI
 * version change.  Conventions as above: caller-owned device buffers, enqueue only, no synchronisation or allocation,
 * argument checks before any HIP call.  No workspace.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_SURFELS_FRAME_CAMERA 0      /* P_cc */
#define SRH_SURFELS_FRAME_WORLD 1       /* P_wc */

typedef struct SrhSurfelsParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24; N = W H pixels per view */
  int32_t frame;                /* SRH_SURFELS_FRAME_* */
  double fovy, focal_length;    /* shared by the views: 0 < fovy < pi, focal_length > 0 */
} SrhSurfelsParams;

/* view (B, 12) fp64: each view's camera-to-world matrix [R | eye], 3 rows of 4 -- needed for the world frame, not looked
 * at for the camera frame; depth (B, N) fp32; out (B, N, 3) fp32 is written. */
int srh_depth_to_surfels_fwd(const SrhSurfelsParams* params, const double* view, const float* depth, float* out,
                             void* stream);

/* Vector-Jacobian product: g_out (B, N, 3) fp32; grad_depth (B, N) fp32 is WRITTEN, every element once, exactly 0 where
 * depth <= 0. */
int srh_depth_to_surfels_bwd(const SrhSurfelsParams* params, const double* view, const float* depth, const float* g_out,
                             float* grad_depth, void* stream);

/* srh_depth_to_surfels_bwd plus the gradient of the view table (see srh_projection_bwd_view), for the world frame only:
 * grad_view (B, 12) fp64; grad_depth may be NULL = not wanted.  A pixel with depth <= 0 still contributes to column 3:
 * the point is the eye. */
int srh_depth_to_surfels_bwd_view(const SrhSurfelsParams* params, const double* view, const float* depth,
                                  const float* g_out, float* grad_depth, double* grad_view, void* view_workspace,
                                  size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's hard scatter-mean projection, projection_renderer (diffrend/torch/projection_layer.py:88-106), for B
 * views per call: each of the N = W H surfels of a view lands on the pixel nearest to its projection (round half to
 * even; outside the frame, NaN or beyond an int: dropped), and a pixel gets the mean of the values that land on it, 0
 * where none does.  Restated as a gather: no float atomic, fp64 sums in ascending surfel index, fp32 results, values and
 * gradients identical from run to run.  mask is 1 WHERE NOTHING LANDED -- the reference's sense, the opposite of the
 * soft masks of the other projection layers.  Only rgb is differentiable.
 *
 * One forward is three steps, because the ordering is the caller's, as for srh_projection_*:
 *   srh_hard_projection_keys   keys (B, N) int32: the surfel's pixel y W + x, N for a dropped surfel
 *   the caller                 order (B, N) int32: per view a STABLE ASCENDING permutation of that view's keys
 *   srh_hard_projection_fwd    the rest.
 * Added without an ABI version change.  Conventions as above: caller-owned device buffers, enqueue only, no
 * synchronisation or allocation, argument checks before any HIP call.  No workspace.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhHardProjectionParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24; N = W H surfels per view */
  int32_t channels;             /* D in 1..SRH_PROJ_MAX_CHANNELS */
  double fovy, focal_length;    /* shared by the views: 0 < fovy < pi, focal_length > 0 */
} SrhHardProjectionParams;

/* view (B, 12) fp64: each view's world-to-camera matrix, 3 rows of 4; surfels (B, N, 3) fp32; keys (B, N) int32 out */
int srh_hard_projection_keys(const SrhHardProjectionParams* params, const double* view, const float* surfels,
                             int32_t* keys, void* stream);

/* rgb (B, N, D) fp32; keys as srh_hard_projection_keys left them; order: per view a stable ascending permutation of the
 * keys (an entry outside 0..N-1 is skipped).  out (B, N, D) fp32, mask (B, N) bytes (1 = no surfel landed) and count
 * (B, N) int32 (kept for the backward) are written, every element once. */
int srh_hard_projection_fwd(const SrhHardProjectionParams* params, const float* rgb, const int32_t* keys,
                            const int32_t* order, float* out, uint8_t* mask, int32_t* count, void* stream);

/* Vector-Jacobian product: keys and count as the forward left them, g_out (B, N, D) fp32; grad_rgb (B, N, D) fp32 is
 * WRITTEN, every element once, 0 for a dropped surfel. */
int srh_hard_projection_bwd(const SrhHardProjectionParams* params, const int32_t* keys, const int32_t* count,
                            const float* g_out, float* grad_rgb, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's constrained plane fit as a layer of its own, estimate_surface_normals_plane_fit_batched
 * (diffrend/torch/utils.py:926-963), for B views per call: a grid of N = W H arbitrary points per view, row by row, to
 * one unit normal per point with nz > 0.  At centre c, over the 8 neighbours k of the reflected 3 x 3 stencil (dy-major),
 *   u_k = (P_k - P_c) / sqrt(|P_k - P_c|^2 + 3e-10),  a = sum ux^2, b = sum ux uy, d = sum uy^2, r = -(sum ux uz, sum uy uz)
 *   (nx, ny) = adj([[a, b], [b, d]]) r / (a d - b^2 + 1e-12),  n = (nx, ny, 1) / sqrt(nx^2 + ny^2 + 1 + 3e-10).
 * rot (B, 9) fp64, row-major: each view's orthonormal lookat basis R = [x y z]; the stored normal is then R n, the value
 * of cam_to_world_batched(None, n, camera)['normal'].  rot = NULL: the camera frame, n as it is.  The rotation is not
 * differentiable.  fp64 arithmetic, one fp32 store per element, no atomic, every element written once, results
 * identical from run to run, and a view's result does not depend on its batch.  Reflection cannot pad a side of 1:
 * W, H >= 2.  Added without an ABI version change.  Conventions as above: caller-owned device buffers, enqueue only, no
 * synchronisation or allocation, argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
/* Bytes of the backward's workspace (five fp64 per point: the gradients of the fit's moments), never 0 for valid sizes;
 * 0 and srh_last_error for n_views outside 1..65535, a side below 2 or W H > 2^24. */
size_t srh_normals_workspace_bytes(int32_t n_views, int32_t width, int32_t height);

/* pos (B, N, 3) fp32; out (B, N, 3) fp32 is written.  No workspace. */
int srh_normals_fwd(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos, float* out,
                    void* stream);

/* Vector-Jacobian product: g_out (B, N, 3) fp32 (with rot, taken back through R^T first); grad_pos (B, N, 3) fp32 is
 * WRITTEN, every element once, all three components.  workspace: 8-byte aligned, srh_normals_workspace_bytes, contents
 * immaterial before and after. */
int srh_normals_bwd(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos,
                    const float* g_out, void* workspace, size_t workspace_bytes, float* grad_pos, void* stream);

/* srh_normals_bwd plus the gradient of the rotations, for the world frame (rot must be given): out = R n, so
 * d loss / d R = sum_q g_out[q] (x) n[q].  grad_rot (B, 12) fp64, WRITTEN with every element once: entries 0..8 of a
 * view are its 3 x 3 gradient row-major like rot, entries 9..11 exactly 0 (the layout srh_view_grad.h's finish kernel
 * writes for every layer).  grad_pos may be NULL = not wanted, and workspace is then not read.  view_workspace:
 * srh_view_grad_workspace_bytes bytes, 8-byte aligned.  Added without an ABI version change. */
int srh_normals_bwd_view(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos,
                         const float* g_out, void* workspace, size_t workspace_bytes, float* grad_pos, double* grad_rot,
                         void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's frame transforms, world_to_cam[_batched] and cam_to_world[_batched] (diffrend/torch/utils.py:539-647),
 * for B views per call.  Per view, n_pos points (x, y, z[, w]), w = 1 for three columns, and n_normal normals, the two
 * counts independent and either 0 = absent (not both), with one fp64 table each:
 *   out_pos[r]    = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3] w,  r = 0..2;  out_pos[3] = w      P = view_pos
 *   out_normal[j] = (n0 A[0][j] + n1 A[1][j]) + n2 A[2][j],             j = 0..2                       A = view_normal
 * The direction is the caller's choice of tables: world to camera is P = lookat (world-to-camera) with A = lookat_inv
 * (camera-to-world), camera to world the other way round.  Column 3 of A is not read, and nothing is normalised.  fp64
 * arithmetic, one fp32 store per element, no atomic, every element written once, results identical from run to run, and
 * a view's result does not depend on its batch.  Added without an ABI version change.  Conventions as above:
 * caller-owned device buffers, enqueue only, no synchronisation or allocation, argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhFrameParams {
  int32_t n_views;                  /* B in 1..65535 */
  int32_t n_pos, n_normal;          /* 0..2^24 per view, not both 0; 0 = that input is absent */
  int32_t pos_cols, normal_cols;    /* 3 or 4, looked at where the count is not 0 */
} SrhFrameParams;

/* view_pos, view_normal (B, 12) fp64, 3 rows of 4: each NULL only where its input is absent.  pos (B, n_pos, pos_cols),
 * normal (B, n_normal, normal_cols) fp32; out_pos (B, n_pos, 4) and out_normal (B, n_normal, 3) fp32 are written.  The
 * pointers of an absent input are not looked at.  No workspace. */
int srh_frame_transform_fwd(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                            const float* pos, const float* normal, float* out_pos, float* out_normal, void* stream);

/* Vector-Jacobian product: g_pos (B, n_pos, 4), g_normal (B, n_normal, 3) fp32, each needed where its input is there;
 * grad_pos (B, n_pos, pos_cols) and grad_normal (B, n_normal, normal_cols) fp32 are WRITTEN, every element once (column 3
 * of grad_normal exactly 0).  Either may be NULL = not wanted, not both.  The transform is linear: the inputs are not
 * read. */
int srh_frame_transform_bwd(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                            const float* g_pos, const float* g_normal, float* grad_pos, float* grad_normal,
                            void* stream);

/* srh_frame_transform_bwd plus the gradients of the two tables (see srh_projection_bwd_view): grad_view_pos and
 * grad_view_normal (B, 12) fp64, every element written, either NULL = not wanted (not both):
 *   d loss / dP[r][c] = sum g_pos[r] [p, w][c],   d loss / dA[i][j] = sum n[i] g_normal[j], column 3 exactly 0.
 * The table of an absent input gets zeros.  grad_pos and grad_normal may both be NULL.  view_workspace:
 * 2 x srh_view_grad_workspace_bytes(n_views, max(n_pos, n_normal), 1) bytes, 8-byte aligned. */
int srh_frame_transform_bwd_view(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                                 const float* pos, const float* normal, const float* g_pos, const float* g_normal,
                                 float* grad_pos, float* grad_normal, double* grad_view_pos, double* grad_view_normal,
                                 void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's project_surfels and project_image_coordinates (diffrend/torch/projection_layer.py:19-85), for B views
 * of N free points each (N is not tied to the frame).  With (X, Y, Z) the position transform above under the view's
 * world-to-camera table and Zd = Z != 0 ? Z : 1:
 *   plane    = (f X / Zd, f Y / Zd, -Z)
 *   px_coord = (plane_x (-(W - 1) / w) + W / 2, plane_y ((H - 1) / h) + H / 2, -Z),  h = 2 f tan(fovy / 2), w = h W / H
 *   px_idx   = srh_hard_projection_keys' key of the point (the same device function): round-half-even(px_coord_y - 1/2) W
 *              + round-half-even(px_coord_x - 1/2), and W H, the dump slot, outside the frame, for NaN or beyond an int.
 * Same guarantees and conventions as the frame transform.  Added without an ABI version change.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhProjectCoordsParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t n_points;             /* N in 1..2^24 per view */
  int32_t cols;                 /* 3 or 4 columns per point */
  int32_t width, height;        /* W, H >= 1, W H <= 2^24 */
  double fovy, focal_length;    /* shared by the views: 0 < fovy < pi, focal_length > 0 */
} SrhProjectCoordsParams;

/* view (B, 12) fp64: each view's world-to-camera matrix; surfels (B, N, cols) fp32.  plane, px_coord (B, N, 3) fp32 and
 * px_idx (B, N) int32 are written where given: each may be NULL = not wanted, not all three.  No workspace. */
int srh_project_coordinates_fwd(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                float* plane, float* px_coord, int32_t* px_idx, void* stream);

/* Vector-Jacobian product: g_plane, g_coord (B, N, 3) fp32, the upstream gradients of plane and px_coord, either NULL =
 * none (not both); grad_surfels (B, N, cols) fp32 is WRITTEN, every element once.  Where Z == 0 the x and y outputs
 * have exactly zero gradient with respect to Z. */
int srh_project_coordinates_bwd(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                const float* g_plane, const float* g_coord, float* grad_surfels, void* stream);

/* srh_project_coordinates_bwd plus the gradient of the view table, grad_view (B, 12) fp64; grad_surfels may be NULL =
 * not wanted.  view_workspace: srh_view_grad_workspace_bytes(n_views, n_points, 1) bytes, 8-byte aligned. */
int srh_project_coordinates_bwd_view(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                     const float* g_plane, const float* g_coord, float* grad_surfels, double* grad_view,
                                     void* view_workspace, size_t view_workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Nearest points between two point sets: the building block of the reference's hausdorff(u, v)
 * (diffrend/torch/ops.py:112-125) and of a Chamfer loss, for B views per call.  Per view u (n_u, dims) and v (n_v, dims):
 *   d2(i, j) = sum over c, ascending, of (u_i[c] - v_j[c])^2     fp64 on the fp32 inputs: nothing overflows or underflows
 *   idx_u[i] = the j of the smallest d2(i, j),  dist_u[i] = sqrt of it (d2 itself with `squared`);  idx_v, dist_v likewise
 * The running best starts at +inf with index 0, candidates are visited in ascending index and one wins only when its
 * d2 is strictly smaller: an exact tie goes to the lowest index, a NaN or +inf d2 never wins, and a query without a
 * finite candidate gets dist = +inf, idx = 0.  No buffer grows with n_u n_v.  fp64 arithmetic, one fp32 store per
 * element, no atomic, every element written once, results identical from run to run, and a view's result does not
 * depend on its batch.  Added without an ABI version change.  Conventions as above: caller-owned device buffers, enqueue
 * only, no synchronisation or allocation, argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhPointSetParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t n_u, n_v;             /* N, M in 1..2^24 per view */
  int32_t dims;                 /* D in 1..4 columns per point */
  int32_t squared;              /* not 0: squared distances, whose gradient is 2 (u - v) */
} SrhPointSetParams;

/* u (B, N, D), v (B, M, D) fp32.  dist_u (B, N) fp32 / idx_u (B, N) int32 and dist_v / idx_v (B, M) are written.  A side
 * whose two outputs are both NULL is not computed (not both sides); exactly one NULL of a pair is refused. */
int srh_nearest_points_fwd(const SrhPointSetParams* params, const float* u, const float* v, float* dist_u,
                           int32_t* idx_u, float* dist_v, int32_t* idx_v, void* stream);

/* Vector-Jacobian product.  With dir(p, o) = (p - o) / |p - o| (2 (p - o) with `squared`), exactly 0 where the fp64
 * distance is 0 or not finite:
 *   grad_u[i] = g_dist_u[i] dir(u_i, v_idx_u[i]) + sum over { j : idx_v[j] = i }, ascending j, of g_dist_v[j] dir(u_i, v_j)
 * and grad_v likewise.  order_u (B, N) / order_v (B, M) int32: per view a STABLE ASCENDING permutation of idx_u / idx_v
 * (the caller sorts, as for srh_hard_projection_fwd); an index or order entry outside its range is skipped.  g_dist_*
 * (B, N) / (B, M) are fp64 -- the sum of several upstream gradients of one distance (hausdorff's symmetric and directed
 * values) then reaches the kernel unrounded -- and may be NULL = a zero upstream gradient, idx_* / order_* of that side
 * are then not read; order_* is needed only where the OTHER set's gradient is wanted.  grad_u (B, N, D) / grad_v (B, M, D) fp32 may be
 * NULL = not wanted (not both), else WRITTEN, every element once; fp64 sums in a fixed order. */
int srh_nearest_points_bwd(const SrhPointSetParams* params, const float* u, const float* v, const int32_t* idx_u,
                           const int32_t* idx_v, const int32_t* order_u, const int32_t* order_v, const double* g_dist_u,
                           const double* g_dist_v, float* grad_u, float* grad_v, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Uniform surface samples of a triangle mesh: the reference's uniform_sample_mesh
 * (diffrend/utils/sample_generator.py:157-194) for B views per call, with the gradient of the samples with respect to
 * the vertices.  Per view v (n_vertices, 3) fp32 and f (n_faces, 3) int32; with p0, p1, p2 the vertices of a face:
 *   n      = c / |c|, c = (p1 - p0) x (p2 - p0), the divisor 1 where |c| = 0
 *   weight = the reference's double area where it is finite and positive, the indices are inside [0, n_vertices) and,
 *            with an eye, n . (eye - p0) >= 0; else 0
 *   cdf    = the running sum of the weights over the view's total, in an order that depends on n_faces alone
 *   face   = the number of faces whose cdf is <= r0;  q = sqrt(s), bary = (1 - q, (1 - t) q, t q)
 *   pos    = (b0 p0 + b1 p1) + b2 p2,  normal = n of the face
 * for the sample's three uniforms (r0, s, t) in [0, 1).  A zero-weight face is never chosen.  A view without a positive
 * weight gets face = -1 and NaN pos, normal and bary, and a zero gradient.  fp64 arithmetic on the fp32 vertices, one
 * fp32 store per element, no atomic, every element written once, results identical from run to run, and a view's result
 * does not depend on its batch.  Added without an ABI version change.  Conventions as above: caller-owned device
 * buffers, enqueue only, no synchronisation or allocation, argument checks before any HIP call.  The caller guarantees
 * 0 <= f < n_vertices and uniforms in [0, 1); a face with an index outside the range has weight 0 and is not read.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct SrhMeshSampleParams {
  int32_t n_views;              /* B in 1..65535 */
  int32_t n_vertices;           /* V in 1..2^24 per view */
  int32_t n_faces;              /* F in 1..2^24 */
  int32_t n_samples;            /* S in 1..2^24 per view */
  int32_t faces_per_view;       /* not 0: f is (B, F, 3), else (F, 3) shared by the views */
  int32_t eye_per_view;         /* not 0: eye is (B, 3), else (3) shared by the views */
} SrhMeshSampleParams;

#define SRH_MESH_WS_FWD 0               /* scratch of srh_mesh_sample_fwd: the cdf, B F fp64, and the views' totals */
#define SRH_MESH_WS_BWD 1               /* scratch of srh_mesh_sample_bwd: the corner gradients, 9 B F fp64 */

/* Bytes of a workspace; 0 for parameters out of range.  Nothing in either outlives its call. */
size_t srh_mesh_sample_workspace_bytes(const SrhMeshSampleParams* params, int32_t which);

/* eye (3) or (B, 3) fp64, NULL = no backface cull; uniforms (B, S, 3) fp64.  pos, normal, bary (B, S, 3) fp32 and face
 * (B, S) int32 are written. */
int srh_mesh_sample_fwd(const SrhMeshSampleParams* params, const float* v, const int32_t* f, const double* eye,
                        const double* uniforms, void* workspace, size_t workspace_bytes, float* pos, float* normal,
                        int32_t* face, float* bary, void* stream);

/* Vector-Jacobian product with face and bary held fixed.  face as the forward wrote it; sample_order (B, S) int32: per
 * view a STABLE ASCENDING permutation of face; corner_order (3 F) int32, or (B, 3 F) with faces_per_view: a stable
 * ascending permutation of the flattened f (the caller sorts, as for srh_hard_projection_fwd); an order entry outside
 * its range is skipped.  g_pos, g_normal (B, S, 3) fp32, either NULL = a zero upstream gradient whose terms are skipped
 * (not both).  The normal's gradient goes through c / |c| and is exactly 0 where |c| is 0 or not finite.  grad_v
 * (B, V, 3) fp32 is WRITTEN, every element once, exactly 0 for a vertex no face references; fp64 sums in ascending
 * sample index per face and ascending corner index 3 face + c per vertex. */
int srh_mesh_sample_bwd(const SrhMeshSampleParams* params, const float* v, const int32_t* f, const double* uniforms,
                        const int32_t* face, const int32_t* sample_order, const int32_t* corner_order,
                        const float* g_pos, const float* g_normal, void* workspace, size_t workspace_bytes,
                        float* grad_v, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * SH9 environment lighting: the reference's radiance_SH9 and irradiance (diffrend/numpy/sph.py:46-138) for B views per
 * call, with their gradients.
 *   Projection.  envmap (B, H, W, C) fp32 -> L (B, C, 9) fp32.  Pixel (i, j), the reference's swapped scales kept:
 *     v = (W/2 - i) / (W/2), u = (j - H/2) / (H/2), r = sqrt(u^2 + v^2), theta = pi r, phi = atan2(v, u)
 *     domega = (2 pi / W) (2 pi / H) sin(pi theta) / (pi theta), the quotient 1 at theta = 0
 *     L[c][k] = sum over the pixels with r <= 1 of (envmap[i][j][c] Y_k) domega, Y_k the nine real harmonics of
 *     (cos phi sin theta, sin phi sin theta, cos theta) in the order (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2)
 *   A pixel with r > 1 is not read: whatever it holds reaches no coefficient, and its gradient is exactly 0.
 *   Irradiance.  M (B, 4, 4, C) fp32, or (4, 4, C) shared by the views, and normal (B, N, 3) fp32 -> E (B, N, C) fp32:
 *     E_c = [n, 1]^T M_c [n, 1] for any M, symmetric or not; n is not normalised.
 * fp64 arithmetic on the fp32 inputs, no atomic, every element written once, sums in an order that depends on H W or N
 * alone: results are identical from run to run, and a view's result does not depend on its batch.  Added without an ABI
 * version change.  Conventions as above: caller-owned device buffers, enqueue only, no synchronisation or allocation,
 * argument checks before any HIP call.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SRH_SH9_MAX_CHANNELS 4

typedef struct SrhSh9Params {
  int32_t n_views;              /* B in 1..65535 */
  int32_t height, width;        /* the probe's H, W, H W in 1..2^24: read by the projection's entry points only */
  int32_t n_points;             /* N in 1..2^24 normals per view: read by the irradiance's entry points only */
  int32_t channels;             /* C in 1..4 */
  int32_t m_per_view;           /* not 0: M is (B, 4, 4, C), else (4, 4, C) shared by the views */
} SrhSh9Params;

#define SRH_SH9_WS_PROJECT 0            /* scratch of srh_sh9_project_fwd: 9 C fp64 per workgroup of 256 pixels */
#define SRH_SH9_WS_IRRADIANCE_BWD 1     /* scratch of srh_sh9_irradiance_bwd with grad_M: 10 C fp64 per workgroup and view */

/* Bytes of a workspace; 0 for parameters out of range.  Nothing in either outlives its call. */
size_t srh_sh9_workspace_bytes(const SrhSh9Params* params, int32_t which);

/* L (B, C, 9) fp32 is written. */
int srh_sh9_project_fwd(const SrhSh9Params* params, const float* envmap, void* workspace, size_t workspace_bytes,
                        float* L, void* stream);

/* g_L (B, C, 9) fp32.  grad_envmap (B, H, W, C) fp32 is WRITTEN, every element once: domega sum_k Y_k g_L[c][k] inside
 * the disc, exactly 0 outside. */
int srh_sh9_project_bwd(const SrhSh9Params* params, const float* g_L, float* grad_envmap, void* stream);

/* E (B, N, C) fp32 is written. */
int srh_sh9_irradiance_fwd(const SrhSh9Params* params, const float* M, const float* normal, float* E, void* stream);

/* Vector-Jacobian product.  g_E (B, N, C) fp32.  grad_normal (B, N, 3) fp32 and grad_M may be NULL = not wanted (not
 * both), else WRITTEN, every element once:
 *   grad_normal = sum_c g_E[c] ((M33_c + M33_c^T) n + M_c[:3, 3] + M_c[3, :3])
 *   grad_M[r][s][c] = sum over the normals of g_E[c] h_r h_s, h = [n, 1]        fp64: (B, 4, 4, C), or (4, 4, C) for a shared
 *                     M, the views' sums added in ascending view order
 * grad_M is fp64 so that a chain behind it (the nine-to-sixteen map from L) sums unrounded values.  The workspace is
 * needed with grad_M only; without it the kernel variant without the reduction runs. */
int srh_sh9_irradiance_bwd(const SrhSh9Params* params, const float* M, const float* normal, const float* g_E,
                           float* grad_normal, double* grad_M, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRH_H */
