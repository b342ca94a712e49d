/*
 * crt_hip.h -- C ABI of libcrt_hip.so, the MI355X (gfx950) drop-in for the reference's per-pixel
 * render loop.  Plain C, plain pointers and sizes; no C++/torch types cross this boundary.
 *
 * R/ = /root/reference/DirectX-RayTracer/DirectX-RayTracer/.  The reference has no FFI: its seam is the
 * C++ class DXRTRenderer (R/DXRTRenderer.h:74-94) plus the CRT* scene layer it owns.  Every entry point
 * below names the reference member it stands in for; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions: every function returning int returns CRT_OK (0) or a CRT_E* code and records a message
 * retrievable with crt_last_error().  The reference reports failure with assert()/ignored HRESULTs
 * (R/DXRTRenderer.cpp:75,113,130,...); the error code replaces that.  A context is used from one host
 * thread at a time (the reference is single threaded, R/DXRTApp.cpp:109-120).  The caller owns every host
 * buffer it passes; the context owns all device memory.  There is NO CPU fallback: without a usable HIP
 * device crt_create() fails with CRT_ENODEVICE.
 */
#ifndef CRT_HIP_H
#define CRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 1

enum {
    CRT_OK = 0,
    CRT_EINVAL = 1,    /* bad argument */
    CRT_ENODEVICE = 2, /* no HIP device / HIP runtime error at init */
    CRT_EHIP = 3,      /* HIP runtime error */
    CRT_ENOMEM = 4,
    CRT_ESTATE = 5,    /* call order (e.g. render before upload) */
    CRT_EIO = 6,       /* scene file */
    CRT_EPARSE = 7
};

#define CRT_MISS 0xFFFFFFFFu
/* shading modes: 0..6 are the reference's closest-hit modes (R/HLSL/ray_tracing_shaders.hlsl:78-169,
 * UI names R/DXRTMainWindow.cpp:100-106; any value in 6..99 behaves as 6, like the shader's final else).
 * >= 100 are extensions that do not exist in the reference. */
#define CRT_MODE_RANDOM_TRIANGLE 0u
#define CRT_MODE_OBJECT_CELLS 1u
#define CRT_MODE_OBJECT_TRIANGLE 2u
#define CRT_MODE_BARYCENTRIC 3u
#define CRT_MODE_HEIGHT 4u
#define CRT_MODE_DISTANCE 5u
#define CRT_MODE_CHECKER 6u
#define CRT_MODE_LAMBERT 100u /* Lambert (+ optional Phong highlight, options "phong_ks" / "phong_exponent") + one shadow ray per light
                                 (BASELINE.json north_star: "Lambert/Phong shading") */
#define CRT_MODE_AMBIENT 120u /* ambient occlusion: the cosine-weighted share of the hemisphere over the hit point that option "ao_samples"
                                 any-hit rays see free within option "ao_radius", as a grey value or (option "ao_sky") as a sky of the
                                 miss colour on top of mode 100's point lights; the contract is below ("ambient occlusion") */
#define CRT_MODE_WHITTED 150u /* mode 100 seen through mirrors and glass: REFLECTIVE and REFRACTIVE surfaces are followed as mode 200
                                 follows them (no Fresnel split, no random numbers, no samples), at most option "max_bounces" turns,
                                 and mode 100 shades the first surface that is neither; the contract is below ("Whitted shading").
                                 101..119, 121..149 and 151..199 behave as 100, every mode >= 200 as 200 */
#define CRT_MODE_PATH 200u    /* path tracing: options "spp" (default 4), "max_bounces" (3), "seed" (1234); BASELINE.json configs[4] */

/* ---- geometry handed over at upload: exactly what createVertexBuffers / createIndexBuffers memcpy ----
 * (R/DXRTRenderer.cpp:391-392,411 and :314-315,334): float xyz stride 12, uint32 indices, mesh ordinal
 * = InstanceID (R/DXRTRenderer.cpp:696). */
typedef struct crt_mesh_view {
    const float* xyz;      /* n_vertices * 3                                  (CRTMesh::getVertices) */
    const uint32_t* idx;   /* n_triangles * 3                                 (CRTMesh::getIndices) */
    const float* normals;  /* n_vertices * 3 or NULL                          (CRTMesh::getVertexNormals) */
    const float* uvs;      /* n_vertices * 3 (u, v, unused) or NULL           (CRTMesh::getUV) */
    uint32_t n_vertices;
    uint32_t n_triangles;
    int32_t material_index; /*                                                (CRTMesh::getMaterialIndex) */
} crt_mesh_view;

typedef struct crt_light { float pos[3]; float intensity; } crt_light;                 /* R/CRTLight.h:4-16 */
typedef struct crt_material { float albedo[3]; uint32_t type; uint32_t smooth; float ior; int32_t texture; } crt_material; /* R/CRTMaterial.h:4-36;
    type = CRTMaterialType; texture = index into crt_set_textures' array when CRTMaterial::isTexture(), else -1 */
/* R/CRTTexture*.h: type 0 albedo (color_a), 1 edges (color_a = edge colour, color_b = inner colour, scalar = edge width; evaluated
 * on the hit's barycentrics), 2 checker (color_a / color_b, scalar = square size), 3 bitmap (pixels: height x width x channels
 * bytes, channels >= 3, nearest texel, v flipped); 2 and 3 are evaluated on the mesh uvs interpolated at the hit,
 * uv0 * (1 - u - v) + uv1 * u + uv2 * v, and at (0, 0) when no mesh of the scene carries uvs (a mesh without uvs among meshes
 * with them has zero uvs).  A material's texture replaces its albedo whatever its type, if 0 <= texture < n_textures;
 * any other index leaves the material's own albedo.
 * Texture conversions: wherever a texture function turns a float into an int (the checker's width = 1 / square_size and its
 * cell numbers floor(u * width), floor(v * width); the bitmap's row (1 - v) * (height - 1) and column u * (width - 1) after u
 * and v are clamped to [0, 1], NaN clamping to 0) the value is truncated towards zero, saturated to [INT_MIN, INT_MAX], and
 * NaN becomes 0.  The checker shows color_a where the wrapped 32-bit sum of its two cell numbers is even ((cu ^ cv) & 1 == 0).
 * So uvs and square sizes of any value, infinities and NaN included, give the same colour on the device, in the host scene
 * layer (crt_scene_texture_color) and in the CPU oracle: square_size 0 (a scene file without the key) is width INT_MAX,
 * square_size > 1 is width 0 (color_a everywhere), a negative one mirrors the cells.  The reference leaves these cases
 * undefined (a plain C++ cast); inside the int range the rule is the reference's. */
enum { CRT_TEX_ALBEDO = 0, CRT_TEX_EDGES = 1, CRT_TEX_CHECKER = 2, CRT_TEX_BITMAP = 3 };
typedef struct crt_texture { uint32_t type; float color_a[3]; float color_b[3]; float scalar; const uint8_t* pixels; uint32_t width, height, channels; } crt_texture;

/* 64-byte BVH node and 48-byte leaf-ordered triangle/shading records as they sit in HBM */
typedef struct crt_bvh_node {
    float lx0, lx1, ly0, ly1, rx0, rx1, ry0, ry1, lz0, lz1, rz0, rz1;
    int32_t left, right; /* >= 0 inner node index; < 0 leaf: ~ref = (first_tri << 3) | count */
    int32_t pad0, pad1;
} crt_bvh_node;
/* 128-byte wide node (full-precision child boxes; the builders' output, host side): up to 4 children, planes stored per axis across the children; collapsed from
 * the binary tree above. ref >= 0: wide node index; negative: leaf (as above).  An unused slot is CRT_BVH_EMPTY = the leaf
 * of no triangles (~0); here its box is inverted (+inf, -inf), in the quantised node it is a single point.  Traversal has no
 * separate test for it: a ray misses the point like any other box it does not pass through, and a ray that did pass exactly
 * through it would visit a leaf without triangles. */
#define CRT_BVH_EMPTY ((int32_t)-1)
typedef struct crt_bvh_node4 {
    float minx[4], maxx[4], miny[4], maxy[4], minz[4], maxz[4];
    int32_t ref[4];
    int32_t pad[4];
} crt_bvh_node4;
/* 64-byte quantised form of the wide node -- what sits in HBM and what the kernels traverse.  lo = minimum corner of the
 * node's own box (union of its children), s = per-axis quantum; child k's box on axis a is
 * [fma(qlo_a.byte[k], s_a, lo_a), fma(qhi_a.byte[k], s_a, lo_a)], rounded outwards (it always contains the full-precision
 * box of crt_bvh_node4), so traversal results are unchanged and only the fetch counts differ by a percent or two.
 * Derived from crt_bvh_node4 by a fixed rule (DESIGN.md "Quantised nodes"; csrc/bvh_build.cpp quantizeBvh4 and the
 * oracle's restatement agree byte for byte).  Unused slots: ref = CRT_BVH_EMPTY, qlo = qhi = 0: the point at the node's minimum
 * corner (a valid box, so the min/max form of the slab test and the octant-specialised one agree on it as on any other). */
typedef struct crt_bvh_node4q {
    float lo[3];
    float s[3];
    uint32_t qlo_x, qhi_x, qlo_y, qhi_y, qlo_z, qhi_z; /* byte k (bits 8k..8k+7) = child k */
    int32_t ref[4];
} crt_bvh_node4q;
typedef struct crt_bvh_tri { float v0[3]; uint32_t inst; float e1[3]; uint32_t prim; float e2[3]; uint32_t gid; } crt_bvh_tri;
typedef struct crt_bvh_shade { float n0[3], n1[3], n2[3]; uint32_t material; uint32_t pad[2]; } crt_bvh_shade;
typedef struct crt_bvh_uv { float uv0[2], uv1[2], uv2[2]; } crt_bvh_uv; /* 24 B, leaf order, only when some mesh has uvs */

typedef struct crt_frame_stats {
    double kernel_ms;        /* HIP-event time of the render kernel(s) on the context's stream */
    double total_ms;         /* wall time of the call (includes D2H copies when host outputs are requested) */
    uint64_t rays_primary;   /* closest-hit rays: pixels rendered by this call (x spp + bounce rays in mode 200, exact when counting) */
    uint64_t rays_shadow;    /* counted only when counting is enabled, else 0 */
    uint64_t nodes_visited;  /* idem: 64-byte quantised wide-node records fetched, summed over all rays */
    uint64_t tris_tested;    /* idem: 48-byte triangle records fetched */
} crt_frame_stats;

typedef struct crt_ctx crt_ctx;

/* ---------------------------------------------------------------------------------------------------
 * Renderer: stands in for DXRTRenderer (R/DXRTRenderer.h:74-94)
 * ------------------------------------------------------------------------------------------------- */

/* DXRTRenderer::prepareForRendering minus window/swap chain (R/DXRTRenderer.cpp:44-62): bind to one HIP
 * device (one process per GPU), create the stream and timing events. */
int crt_create(crt_ctx** out, int device_id);
void crt_destroy(crt_ctx* ctx);
const char* crt_last_error(const crt_ctx* ctx); /* ctx may be NULL: last error of a failed crt_create */
uint32_t crt_abi_version(void);

/* createVertexBuffers + createIndexBuffers + createAccelerationStructures
 * (R/DXRTRenderer.cpp:379-453, 302-376, 548-806): copies geometry, builds the BVH on the host (binned SAH)
 * and uploads nodes / leaf-ordered triangles / shading records to HBM.  A second call replaces the scene.  Vertices and
 * per-mesh transforms can change afterwards when option "dynamic" was set before the upload (crt_update_vertices and the
 * functions beside it, below); triangles, indices, uvs and materials need a new upload. */
int crt_upload_scene(crt_ctx* ctx, const crt_mesh_view* meshes, uint32_t n_meshes,
                     const crt_light* lights, uint32_t n_lights,
                     const crt_material* materials, uint32_t n_materials);

/* textures the materials refer to by index (CRTScene::getTextures / getTextureByName, R/CRTScene.h:32-34); copied, pixels
 * included; may be called before or after crt_upload_scene. The reference parses them but its renderer never samples
 * them; here they drive the albedo of modes 100 and 200 */
int crt_set_textures(crt_ctx* ctx, const crt_texture* textures, uint32_t n_textures);

/* updateCameraCB (R/DXRTRenderer.cpp:248-270): position + 3x3 row-major rotation, dirWorld = R * dirCam */
int crt_set_camera(crt_ctx* ctx, const float pos[3], const float rot3x3_rowmajor[9]);
/* changeShadingMode (R/DXRTRenderer.cpp:1359-1363) */
int crt_set_shading_mode(crt_ctx* ctx, uint32_t mode);
/* miss colour; default (0,1,1) = the reference's miss shader (hlsl:72-76) */
int crt_set_miss_color(crt_ctx* ctx, const float rgb[3]);
/* when enabled the render kernels also count node/triangle fetches and shadow rays (slower variant) */
int crt_set_counting(crt_ctx* ctx, int enabled);

/* renderFrame (R/DXRTRenderer.cpp:1370-1408), synchronous like the reference (fence wait :521-527).
 * Host outputs, any may be NULL: rgba8 w*h*4 (R8G8B8A8_UNORM, row-major, top-left origin), hit_inst / hit_prim
 * w*h uint32 (CRT_MISS on miss), hit_t w*h float, rgb_f32 w*h*3 float (pre-quantisation colour). */
int crt_render_frame(crt_ctx* ctx, uint32_t width, uint32_t height,
                     uint8_t* rgba8, uint32_t* hit_inst, uint32_t* hit_prim, float* hit_t, float* rgb_f32,
                     crt_frame_stats* stats);

/* Same frame, outputs left in HBM: device pointers (any may be NULL except d_rgba8). Asynchronous on the
 * context's stream unless stats != NULL (then it synchronises to read the timers). */
int crt_render_frame_device(crt_ctx* ctx, uint32_t width, uint32_t height,
                            void* d_rgba8, void* d_hit_inst, void* d_hit_prim, void* d_hit_t, void* d_rgb_f32,
                            crt_frame_stats* stats);

/* ---- tile-partitioned rendering for N GPUs (no reference counterpart) ----------
 * The frame is cut into 16x16-pixel macro tiles, numbered row-major; macro tile k belongs to rank k % n_ranks.
 * A rank renders its tiles into a rank-contiguous, tile-major staging buffer: slot j (= k / n_ranks) holds
 * 256 RGBA8 pixels (row-major inside the tile; pixels outside the frame are left untouched).  All ranks use the
 * same slot count crt_tile_slots() so the per-rank buffers can be gathered with one RCCL all-gather/gather. */
uint32_t crt_tile_count(uint32_t width, uint32_t height);
uint32_t crt_tile_slots(uint32_t width, uint32_t height, uint32_t n_ranks); /* ceil(tile_count / n_ranks) */
int crt_render_tiles_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks,
                            void* d_staging_rgba8 /* slots*256*4 bytes */, crt_frame_stats* stats);
/* Throughput mode (no reference counterpart: DXRTRenderer::renderFrame issues one DispatchRays per call, R/DXRTRenderer.cpp:1348-1350):
 * n_frames (1..4) frames of the current scene, mode and size in ONE launch.  A launch lasts as long as its slowest 8x8 packet
 * (a grazing ray walks hundreds of dependent steps); a batch shares that critical path, which is what bounds an N-GPU tile
 * share (1/N of the work, same critical path).  cameras = n_frames x 12 floats {pos[3], rot3x3_rowmajor[9]} or NULL (the
 * current camera for every frame); d_rgba8[f] / d_staging[f] = frame f's output, laid out as in crt_render_frame_device /
 * crt_render_tiles_device.  Frames are independent: each equals what a single-frame call with its camera renders. */
int crt_render_frames_batch_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_frames, const float* cameras,
                                   void* const* d_rgba8, crt_frame_stats* stats);
int crt_render_tiles_batch_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks, uint32_t n_frames,
                                  const float* cameras, void* const* d_staging, crt_frame_stats* stats);

/* De-interleave a gathered buffer (n_ranks * slots * 1024 bytes, rank-major) into a row-major frame. */
int crt_untile_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_ranks,
                      const void* d_gathered, void* d_rgba8_rowmajor);
/* the same for frame `frame` of an all-gathered BATCH: when each rank sends its n_frames staging buffers as one contiguous
 * message (n_frames x crt_tile_slots() tiles), d_gathered holds n_ranks x n_frames x crt_tile_slots() tiles */
int crt_untile_batch_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_ranks, uint32_t n_frames, uint32_t frame,
                            const void* d_gathered, void* d_rgba8);

/* ---- native RCCL frame assembly: the N-GPU frame without Python (no reference counterpart: the reference is one GPU, one
 * DispatchRays, R/DXRTRenderer.cpp:1346-1350, 1405).  One process per GPU, each with its own context and the same scene.
 * Rank 0 calls crt_comm_unique_id and hands the 128 bytes to the other ranks (file, pipe, MPI: the caller's business); every
 * rank calls crt_comm_init (collective: returns when all n_ranks have called it).  crt_render_frame_distributed then renders
 * this rank's macro tiles (crt_render_tiles_device), moves them with ONE ncclAllGather over xGMI -- crt_tile_slots() * 1024 bytes
 * per rank: 1 044 480 B at 1920x1080 on 8 GPUs, 4 177 920 B on 2 -- and de-interleaves the gathered
 * buffer; every rank ends up with the whole frame.  Asynchronous on the context's stream unless stats or host_rgba8 is given.
 * d_rgba8: device frame (w*h*4 bytes) or NULL (a context-owned buffer is used); host_rgba8: optional host copy.
 * RCCL is loaded at run time (librccl.so.1): a process that never calls these needs no RCCL. */
#define CRT_COMM_ID_BYTES 128
int crt_comm_unique_id(void* id_out /* CRT_COMM_ID_BYTES */);
int crt_comm_init(crt_ctx* ctx, uint32_t rank, uint32_t n_ranks, const void* unique_id);
/* The same frame assembly with shared host memory as the transport, for ranks that share ONE GPU (RCCL refuses that: rehearsing the
 * multi-rank path on a one-GPU machine) or where RCCL cannot be loaded: `name` ("/something") names a POSIX shared-memory object
 * that rank 0 creates and removes; collective like crt_comm_init.  Per frame every rank copies its tiles into the object, waits for
 * the others, and copies all tiles out.  Correct, slow, never a measurement. */
int crt_comm_init_host(crt_ctx* ctx, uint32_t rank, uint32_t n_ranks, const char* name);
int crt_comm_destroy(crt_ctx* ctx);
int crt_comm_info(const crt_ctx* ctx, uint32_t* rank, uint32_t* n_ranks); /* n_ranks = 0: no communicator */
int crt_render_frame_distributed(crt_ctx* ctx, uint32_t width, uint32_t height, void* d_rgba8, uint8_t* host_rgba8, crt_frame_stats* stats);

/* options. Phong term of mode 100: the reference's CRTMaterial has no specular coefficient or exponent
 * (R/CRTMaterial.h:30-35 holds type, albedo, smooth_shading, ior, texture), so both are renderer-wide options invented here:
 * "phong_ks" = specular coefficient in thousandths (0 = off, the default; 300 = 0.3), "phong_exponent" = integer exponent
 * 1..65536 (default 32).  Per unoccluded light: rgb += ks * intensity / (4 pi r^2) * max(0, R . V)^n, R = light direction
 * mirrored about the shading normal, V = direction to the eye; white highlight, x^n by square and multiply.
 * "gpu_build" 0/1: acceleration structure built on the GPU at the next crt_upload_scene.  "gpu_builder" picks the GPU builder for
 * those uploads and for crt_rebuild: 0 = LBVH (the default), 1 = PLOC (closer to the SAH tree in quality, slower to build); other
 * values -> CRT_EINVAL.  It has no effect on host SAH uploads.
 * Rendering parameters of mode 200: "spp", "max_bounces", "seed" ("max_bounces" also limits the turns of mode 150).
 * Rendering parameters of mode 120: "ao_samples" (1..4096, default 16), "ao_radius" (0..1000000 thousandths of the scene box's
 * diagonal, default 0 = unbounded), "ao_sky" (0/1, default 0) and "seed"; other values -> CRT_EINVAL ("ambient occlusion" below). Tuning knobs (speed only, results never
 * change): "inner_min" / "inner_min_any" wave scheduling of the closest-hit / any-hit traversal loops (1..65: node steps while that
 * many lanes stand on inner nodes; -1..-8: while that many eighths of the wavefront's live lanes do; default -6), "xcd_group", "adaptive_order" (launch the most expensive 8x8
 * packets of the previous frame first: 0 never, 1 always, 2 = default: only for a frame issued on the same stream as the frame
 * before, where frames run one after another), "remeasure_every" (a moving camera re-measures packet costs every n-th use of a scratch slot; default 1), "boost_units",
 * "split_units" (with a launch order: the n most expensive 8x8 packets are rendered by several wavefronts each, whose lanes
 * share the pieces of the block's rays -- same frame, shorter critical path; -1 = automatic, the default: none for a whole frame
 * on one GPU, 64 / 128 packets for the tile share of 2 / >= 4 ranks, whose lone launch goes from 221 / 199 / 178 us to 188 / 132 /
 * 118 us at 2 / 4 / 8 ranks; 0 = off; fetch counters of split packets grow), "split_rays" (16, 8 or 4 rays per wavefront of a
 * split packet, default 4), "split_segments" (4, 8 or 16 pieces per split ray, default 16),
 * "xcd_affine_order" 0/1 (with a launch order: the frame is cut into eight regions of equal cost, one per XCD and its L2, each launched
 * most expensive packet first; default 0 -- primary rays alone gain 5 %, a shaded frame loses 1 %),
 * "path_tile" (mode 200 work split: pixel-tile edge per workgroup, 8 (default, also 0) or 16), "path_pipeline" (mode 200: 0 (default) = one persistent kernel
 * whose wavefronts carry a pixel tile's paths through all stages with private queues; 1 = the stages as separate launches (camera rays,
 * shade + shadow rays, bounce rays, resolve) over global queues: no register spills, 6-7 wavefronts per SIMD instead of 5, identical
 * frames, 8 % slower on the 5M-triangle 4K frame because the compute-bound camera stage no longer overlaps the fetch-bound stream
 * stages; its queues hold "path_pass_paths" paths per pass (65536..2^25, default 2^24 = 1.9 GB), a frame with more is rendered in
 * several passes), "path_ranges" (mode 200: 8 (default) = the
 * work items are cut into eight contiguous ranges and a wavefront works through the range of the XCD it runs on before taking from the others', 1 = one shared work counter), "stack_entries" (0 = default 16; deeper entries spill to a
 * global arena), "wide_offsets" (frames of modes 0..100: 0 (default) = the render kernel computes the byte offset of a node or triangle
 * record in 32 bits whenever 64 * nodes <= 2^32 and 48 * triangles <= 2^32, and in 64 bits otherwise; 1 = always in 64 bits.  Results
 * are the same either way), "list_short_max" (crt_list_hits*: 1..1024, default 24: lists up to this many hits are sorted by one lane, longer ones by a wavefront). The diagnostic options "timeline", "debug_skip_units" and "debug_force_measure" (which do change what a frame
 * does) exist only in the diagnostic build of the library (tools/diag_build.sh); the product returns CRT_EINVAL for them. */
int crt_set_option(crt_ctx* ctx, const char* name, int value);

/* diagnostic build only (the product returns 0 words): with option "timeline" = 1 and counting enabled, a render records per workgroup {start, end} on the
 * 100 MHz s_memrealtime clock and (XCC id << 32 | tile_y << 16 | tile_x); this copies them out (3 words per workgroup) */
int crt_debug_read_timeline(crt_ctx* ctx, unsigned long long* out, size_t max_words, size_t* n_words);
/* raw device counters of the last counting render: [0] nodes [1] triangles [2] shadow rays [3] closest-hit rays; [4..31]
 * are filled only by the CRT_PROF diagnostic build of the kernels (tools/prof_build.sh, meanings in tools/prof_run.py) */
int crt_debug_read_counters(crt_ctx* ctx, unsigned long long out[32]);
/* HIP-event times in ms of the phases of the last crt_list_hits* call that was given stats: [0] count, [1] scan, [2] fill,
 * [3] sort + resolve (fill and sort 0 when the records were not written).  Their sum is that call's kernel_ms less the gaps. */
int crt_debug_list_phases(crt_ctx* ctx, double out_ms[4]);
/* self-check of the device arithmetic the triangle test relies on: its short reciprocal against the correctly rounded
 * 1.0f / d for all 2^32 inputs, on device device_id.  out[0] mismatches (0 expected), [1] inputs checked (2^32), [2..5]
 * mismatches of the unguarded Newton form by class (biased exponent 0 / 253..255 / all-ones significand / the rest), [6]
 * smallest mismatching input or ~0.  Synchronous; a few milliseconds of GPU time. */
int crt_debug_check_rcp(int device_id, unsigned long long out[8]);

/* diagnostics: the render kernel's fetch form for a tree of n_nodes nodes and n_tris triangles under option "wide_offsets" =
 * option: 1 = 64-bit offsets, 0 = 32-bit offsets.  Pure host arithmetic, no device needed. */
int crt_debug_wide_offsets(unsigned long long n_nodes, unsigned long long n_tris, int option);

/* stream plumbing: run on an external hipStream_t (e.g. torch's current stream; NULL = HIP's default stream);
 * crt_reset_stream goes back to the context's private non-blocking stream */
int crt_set_stream(crt_ctx* ctx, void* hip_stream);
int crt_reset_stream(crt_ctx* ctx);
int crt_synchronize(crt_ctx* ctx);

/* BVH introspection (tests, tooling): sizes, then copies of the host-side arrays uploaded to HBM */
int crt_bvh_info(const crt_ctx* ctx, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* max_depth);
int crt_bvh_export(const crt_ctx* ctx, crt_bvh_node* nodes, crt_bvh_tri* tris, crt_bvh_shade* shade);
/* per-triangle texture coordinates in leaf order; *has_uvs = 0 (and nothing copied) when no mesh carried uvs */
int crt_bvh_export_uv(const crt_ctx* ctx, crt_bvh_uv* uvs, int* has_uvs);
/* wall time of the last crt_upload_scene (flatten + build + collapse + upload) and, with option "gpu_build" = 1 (LBVH
 * built by HIP kernels instead of the host SAH builder: 8.7 against 360 ms at 1M triangles, frames over its tree 1.0 .. 1.14 x
 * the SAH tree's), the device time of the build kernels */
int crt_build_stats(const crt_ctx* ctx, double* upload_ms, double* device_build_ms);
/* the wide tree as it sits in HBM: count/depth (any pointer may be NULL), then a copy of the nodes */
int crt_bvh_info4(const crt_ctx* ctx, uint32_t* n_nodes4, uint32_t* depth4);
int crt_bvh_export4(const crt_ctx* ctx, crt_bvh_node4* nodes4);
/* the same nodes in the 64-byte quantised form the kernels fetch (count = n_nodes4) */
int crt_bvh_export4q(const crt_ctx* ctx, crt_bvh_node4q* nodes4q);
/* the decoded plane table beside those nodes: n_nodes4 rows of 32 floats,
 * row i = float(q) of plane byte k of node i (qlo_x .. qhi_z, child j = byte j of each word) for k < 24, then 8 zeros.  The
 * kernels' node steps read it when a whole wavefront stands on one node. */
int crt_bvh_export_planes4q(const crt_ctx* ctx, float* planes);
/* host-only BVH build, no device needed (used by crt_upload_scene; exposed for tests and tooling) */
int crt_bvh_build_host(const crt_mesh_view* meshes, uint32_t n_meshes,
                       crt_bvh_node** nodes, uint32_t* n_nodes,
                       crt_bvh_tri** tris, crt_bvh_shade** shade, uint32_t* n_tris, uint32_t* max_depth);
/* same build, additionally returning the collapsed wide tree (nodes4 freed with crt_free) */
int crt_bvh_build_host4(const crt_mesh_view* meshes, uint32_t n_meshes, crt_bvh_node4** nodes4, uint32_t* n_nodes4, uint32_t* depth4);
/* the quantisation rule alone: n wide nodes -> n quantised nodes (caller-provided output array) */
int crt_bvh_quantize4(const crt_bvh_node4* nodes4, uint32_t n, crt_bvh_node4q* out);
void crt_free(void* p);

/* page-locked host memory for crt_render_frame's output buffers: the device-to-host copy of a frame then runs at PCIe speed
 * instead of through the driver's staging of pageable memory (8.3 MB at 1080p: 0.36 -> 0.17 ms).  Optional: any host
 * pointer works.  Needs a HIP device; NULL on failure.  Release with crt_host_free. */
void* crt_host_alloc(size_t bytes);
void crt_host_free(void* p);

/* ---- progressive accumulation (no reference counterpart: the reference's idle tick renders every frame from scratch,
 * R/DXRTApp.cpp:109-120).  While the view holds still, mode-200 frames add their samples to per-pixel sums, and the image
 * converges instead of showing the same noise on every tick.
 * - Only mode 200 accumulates.  With accumulation on, a mode-200 call traces samples n .. n+spp-1, n = the samples already in
 *   the sums, adds them to per-pixel float64 sums in sample order and outputs the mean of all n+spp samples ((float)(sum / total),
 *   to RGBA8 and, where asked for, f32 rgb).  K calls of S spp therefore equal, bit for bit, one call of K*S spp; spp may
 *   change between calls (4 + 1 + 3 spp = the 8-spp frame).  Other modes ignore the setting: their frames are those rendered
 *   with it off, and they leave the sums untouched.
 * - Limit: a call that would pass max_samples traces only the remainder.  Once the sums hold max_samples, a call traces
 *   nothing: it writes the stored mean again (RGBA8 / f32 rgb; no hit outputs) and its crt_frame_stats report zero rays.
 * - Automatic reset: a mode-200 call starts over at sample 0 when any of these differ from what the sums were made with:
 *   camera pose (compared bitwise: setting the same pose again keeps accumulating), shading mode, miss colour, max_bounces,
 *   seed, the uploaded scene, the textures, width x height, and the entry point kind with its (rank, n_ranks).  spp,
 *   counting and the tuning options (path_pipeline, path_tile, path_ranges, path_pass_paths, ...) do not reset: results never
 *   depend on them.  Mode 200 -> 3 -> 200 with nothing else changed continues the sums.
 * - Hit outputs report the call's first camera sample (global index n; sample 0 after a reset, as without accumulation).
 * - crt_render_frame, crt_render_frame_device and crt_render_tiles_device accumulate, and so does crt_render_frame_distributed
 *   (each rank sums its own tile slots; the gather moves resolved RGBA8 only).  The batch entry points return CRT_EINVAL in
 *   mode 200 with accumulation on and render nothing: their frames have different cameras.
 * - Consecutive accumulating calls run in issue order on the GPU even when issued on different streams (crt_set_stream).
 * The sums are four doubles per output pixel (staging slot pixel for tile shares), owned by the context: allocated by the first
 * accumulating frame (66 MB at 1920x1080, 265 MB at 3840x2160), freed by crt_set_accumulation(ctx, 0) or crt_destroy.  A pixel
 * whose samples are all equal resolves to that value exactly at any count up to the limit. */
int crt_set_accumulation(crt_ctx* ctx, uint32_t max_samples); /* 0 = off (default); 1..2^24 = on, up to that many samples per pixel
                                                                  (2^24: every count is exact in fp32, the sums are float64); always starts over */
int crt_reset_accumulation(crt_ctx* ctx);                      /* drop the sums; the next frame starts at sample 0 */
int crt_accumulated_samples(const crt_ctx* ctx, uint32_t* samples); /* samples per pixel in the current sums (0 when off or reset) */

/* ---- non-finite vertices (inert triangles).  A triangle with a NaN or an infinity among its nine vertex coordinates, as traced
 * (world space for a dynamic scene: a diverged solver's output handed to crt_update_vertices*, finite rest vertices that a
 * crt_set_mesh_transform carries past FLT_MAX), is inert:
 * - no frame, ray query, occlusion query, hit count, all-hits list, occupancy or closest-point query ever reports it;
 * - every result equals the result for the same scene with the inert triangles absent; inst, prim and the global ids of all
 *   other triangles are unchanged (an inert triangle keeps its place in the numbering and in the leaf-ordered records);
 * - this holds over every tree -- host SAH, gpu_build LBVH or PLOC, after crt_refit, after crt_rebuild with either builder --
 *   with the "boundary rays" limit of the ray queries as the only exception, as for finite scenes;
 * - uploads, refits and rebuilds of such scenes succeed (PLOC included), and crt_mesh_vertices returns the non-finite values
 *   as they are.
 * How: where a triangle's box and centroid are taken (every builder, the refit), a triangle with a coordinate x that fails
 * x - x == 0 is the point (0, 0, 0), so no box, Morton code, SAH bin or quantised plane is ever computed from a non-finite
 * number and the boxes above a leaf always hold its finite triangles.  Its leaf-ordered record keeps inst / prim / gid and
 * holds nine quiet NaNs (bits 0x7FC00000) as v0 / e1 / e2, whoever writes it (host build, GPU build, refit, rebuild): the sign
 * that e = v1 - v0 gives a NaN differs between compilers and between host and device code, and the exported bytes must not
 * depend on that.  The Moeller-Trumbore test and the closest-point routine reject such a record by themselves (every
 * comparison with a NaN is false).  A scene of finite vertices gets the trees and records it got before, byte for byte.  Finite coordinates of huge
 * magnitude (extents beyond 3e38) remain unsupported; non-finite normals or uvs are not covered. */

/* ---- batched ray queries (DXR offers TraceRay on any ray; the reference only traces its own camera rays,
 * R/HLSL/ray_tracing_shaders.hlsl:21-69).  The caller hands over rays and asks what they hit: picking, visibility / ambient
 * occlusion rays, sensor casts.
 * - Ray record: 8 floats (32 B) {ox, oy, oz, tmin, dx, dy, dz, tmax}; the buffer holds n records, contiguous.  The direction
 *   need not be normalised: t is in units of |d|.  A hit is a triangle with tmin < t < tmax, by the frames' Moeller-Trumbore
 *   test (two sided, no culling).  tmin may be 0 or negative, tmax may be +inf.  A record containing a NaN, or with
 *   !(tmin < tmax), is not traced and reports a miss / not occluded; a zero direction is a miss.
 * - Direction magnitude: any finite non-zero largest component, 2^-149 .. FLT_MAX.  A record is traced as the same ray
 *   prescaled by a power of two, (o, tmin 2^e, d 2^-e, tmax 2^e) with e the exponent of the largest |d_i|, and t is returned
 *   as t' 2^-e.  The scaling is exact: a record and its 2^k multiple give the same hit, u, v and fetch counts, and t 2^k is
 *   the unscaled t, wherever the scaled values stay normal floats.  Edges: tmin 2^e or tmax 2^e below 2^-126 in magnitude is
 *   rounded; a t that leaves the float range is reported as +inf (still a hit) or as a subnormal; a component below 1e-20 of
 *   the largest counts as +-1e-20 of it in the slab test (a boundary ray, below).  A zero direction, just outside the
 *   range, hits nothing.
 * - Scene scale: the vertices, the origins and tmin / tmax times 2^k (directions as they are) give the same inst, prim, u, v
 *   and occlusion, and t 2^k, bit for bit, while every intermediate stays a normal float.  The Moeller-Trumbore products are
 *   cubic in a length, so that range is about a third of float32's: measured on a scene of extent 4 with edges of 0.1 .. 2 and
 *   257 records (tests/test_scale_similarity.py), k = -34 .. 41 for the closest hit and for all hits,
 *   -43 .. 41 for occlusion, -41 .. 41 for hit counts.  Outside it products go subnormal or overflow and results change
 *   without an error being reported; kernel and oracle still agree bit for bit there (checked at the first k outside).  A scene much smaller than 2^-30 or larger than 2^40 units should be rescaled by the caller.
 * - Closest hit (crt_trace_rays*), per ray, each output optional: t (float), uv (2 floats: u = weight of v1, v = weight of
 *   v2, the frames' barycentrics), inst (uint32 mesh ordinal in upload order), prim (uint32 triangle of that mesh).  Equal t
 *   goes to the lower global triangle id, as in the frames.  Miss: inst = prim = CRT_MISS, t = the ray's tmax, u = v = 0.
 * - Occlusion (crt_occluded_rays*): one byte per ray (the layout of torch.bool / np.bool_), 1 if any triangle lies in
 *   (tmin, tmax): the any-hit traversal with early exit.
 * - Results do not depend on the order of the rays in the buffer, on scheduling or on the tuning options inner_min /
 *   inner_min_any.  The box cull is the frames' (boxes are tested against the best t so far widened by 2^-18 of its
 *   magnitude), so the results and fetch counts are bit for bit the CPU oracle's traversal of that ray.  For a negative bound
 *   the widening keeps its direction (the frames' factor would narrow it): a triangle strictly inside (tmin, tmax) is found,
 *   and ties at t < 0 go to the lower global id, as at t > 0.
 * - Limit (boundary rays): the slab test is conservative against the absolute rounding that comes from the ray origin's
 *   distance to the world origin.  Its near and far distances are padded by 2^-21 |o / d| per axis, so a
 *   box the ray enters is not culled for that reason at any offset.  What remains is the relative rounding of the slab
 *   distances, a few ulps of t.  A triangle whose hit lies where the ray runs within that of a box edge can still be rejected
 *   with its box.  This concerns a ray lying in an axis-aligned face of the boxes (an axis-aligned direction through the
 *   plane of axis-aligned geometry, or through a shared edge of such quads) and a ray starting on a surface whose own hit
 *   is at t ~ tmin.  Such a ray may then report a miss, or a farther hit, although a triangle lies in (tmin, tmax).  The
 *   result is still the oracle's traversal of the same tree, but it can differ between the host SAH tree and the gpu_build
 *   tree.  Every other ray gives the same result over either tree, however far from the origin the scene lies.
 *   Inert triangles (non-finite vertices, above) are never hit and hide nothing, over any tree.
 * - Layout: queries traverse the 64-byte 4-wide tree the frames traverse.
 * - A query needs an uploaded scene (CRT_ESTATE otherwise).  It reads the tree, the triangles and the options inner_min /
 *   inner_min_any, nothing else: camera, mode, accumulation sums, launch-order state and frame outputs are untouched, and a frame
 *   rendered after any number of queries equals the frame rendered without them (accumulating mode-200 runs included).
 * - n = 0 returns CRT_OK and launches nothing (the buffers are not looked at).  Offsets are 64-bit: n up to 2^32 - 1.
 * - stats (may be NULL): kernel_ms = the query kernel (HIP events), total_ms = wall time of the call, rays_primary = n for a
 *   closest-hit query, rays_shadow = n for an occlusion query; nodes_visited / tris_tested with crt_set_counting(ctx, 1), counted
 *   as the frames count them.
 * *_device: device pointers.  The ray buffer must be 16-byte aligned, t / inst / prim 4-byte, uv 8-byte aligned (CRT_EINVAL
 * otherwise).  Any closest-hit output may be NULL, not all four.  Asynchronous on the context's stream (crt_set_stream) unless
 * stats != NULL.  Host variants: synchronous, staged through a context-owned device buffer that grows on demand. */
int crt_trace_rays_device(crt_ctx* ctx, uint32_t n, const void* d_rays, void* d_t, void* d_uv, void* d_inst, void* d_prim,
                          crt_frame_stats* stats);
int crt_occluded_rays_device(crt_ctx* ctx, uint32_t n, const void* d_rays, void* d_occluded, crt_frame_stats* stats);
int crt_trace_rays(crt_ctx* ctx, uint32_t n, const float* rays, float* t, float* uv, uint32_t* inst, uint32_t* prim,
                   crt_frame_stats* stats);
int crt_occluded_rays(crt_ctx* ctx, uint32_t n, const float* rays, uint8_t* occluded, crt_frame_stats* stats);

/* ---- shaded ray queries: colour, normal and albedo for caller-supplied rays (DXR lets any shader call TraceRay and shade
 * the result; the reference only does so from its own rayGen, R/HLSL/ray_tracing_shaders.hlsl:21-169; Open3D's cast_rays
 * returns primitive_normals).  A fisheye or equirectangular sensor, a calibrated lens, a lidar's return intensity, light
 * fields, probes: the frames' shading without the frames' pinhole camera, in one launch.
 * - Rays: the 8-float records of crt_trace_rays, with the same NaN / empty-interval / zero-direction rules and the same range
 *   of direction magnitudes; they are traced prescaled by 2^e in the same way.  The hit is exactly the one crt_trace_rays
 *   reports for that record: t / uv / inst / prim are its outputs bit for bit, each optional.  At least one of the seven
 *   outputs must be non-NULL.
 * - Mode: the context's current shading mode (crt_set_shading_mode) applies.  Modes 0..99 are the seven reference modes
 *   (7..99 behave as 6, as in the frames); mode 100 is Lambert with optional Phong (options "phong_ks", "phong_exponent") and
 *   one shadow ray per light (101..199 behave as 100, except 120: "ambient occlusion", and 150: "Whitted shading", both below).  Mode 200 returns CRT_EINVAL and launches nothing: path tracing of caller rays would need a
 *   sample-indexing contract of its own (crt_path_rays* below has it).
 * - What the shading sees: the record's own origin and direction and the unscaled t (t' 2^-e, the value reported) -- exactly
 *   what the frame kernels hand the same functions for a camera ray.  Nothing is normalised: the hit point is o + d * t per
 *   component, the entering test is the sign of dot(N, d), Phong's view vector is -d.  So a record that holds a frame's camera
 *   ray (origin = the camera position, direction = the unit vector the frame's rayGen produces for the pixel, tmin = 0.001,
 *   tmax = 10000) gives that pixel's rgb_f32 bit for bit.  Mode 5 (a function of t) and the Phong term (of -d) depend on
 *   |d|: a caller who wants the frames' semantics passes unit directions.
 * - Shadow rays of mode 100 are the frames': origin = the hit point moved 1e-3 along the shading normal, unit direction to the
 *   light, interval (0, distance), boxes culled against distance (1 + 2^-18); traced only for a positive cosine, in light
 *   order, and accumulated with the frames' fmaf sequence.  They are not prescaled (their direction is a unit vector).
 * - rgb (3 floats per ray): on a hit the mode's colour before quantisation; on a miss or an untraced record the miss colour
 *   (crt_set_miss_color).
 * - normal (3 floats per ray): the shading normal of the frames' surface evaluation -- normalised, flipped to face the ray;
 *   the geometric normal when the material is flat or the mesh has no usable vertex normals.  Miss: (0, 0, 0).
 * - albedo (3 floats per ray): the material's colour, or its texture's colour where it has one; (1, 1, 1) for a material
 *   index out of range, as in the frames.  Miss: (0, 0, 0).
 * - normal and albedo are available in every mode 0..100; a debug mode evaluates the surface only when one of them is asked for.
 * - Pending refits are applied first.  Camera, mode, accumulation sums, launch orders and frame outputs are untouched.
 *   Results do not depend on the order of the records, on scheduling or on the options inner_min, inner_min_any and
 *   stack_entries.  The boundary-ray limit of the ray queries applies unchanged; inert triangles are never hit and never
 *   occlude.
 * - n = 0 returns CRT_OK and launches nothing.  CRT_ESTATE without a scene.  CRT_EINVAL for a NULL ctx, NULL rays with n > 0,
 *   all outputs NULL, mode 200, or a misaligned device pointer (rays 16-byte, uv 8-byte, everything else 4-byte).  These
 *   checks come before the refit: a failed call launches nothing.
 * - stats (may be NULL): kernel_ms, total_ms, rays_primary = n; with crt_set_counting(ctx, 1) rays_shadow = the shadow rays
 *   traced and nodes_visited / tris_tested = the closest-hit and shadow traversals together, counted as the frames count
 *   them: for a buffer of a frame's camera rays they are the oracle's statistics of that frame in that mode.
 * *_device: device pointers, asynchronous on the context's stream (crt_set_stream) unless stats != NULL.  Host variant:
 * synchronous, staged through the context's query staging buffer. */
int crt_shade_rays_device(crt_ctx* ctx, uint32_t n, const void* d_rays, void* d_rgb, void* d_normal, void* d_albedo, void* d_t,
                          void* d_uv, void* d_inst, void* d_prim, crt_frame_stats* stats);
int crt_shade_rays(crt_ctx* ctx, uint32_t n, const float* rays, float* rgb, float* normal, float* albedo, float* t, float* uv,
                   uint32_t* inst, uint32_t* prim, crt_frame_stats* stats);

/* ---- Whitted shading (CRT_MODE_WHITTED, 150): mirrors and glass without path noise.  No function of its own: in mode 150
 * crt_shade_rays* and crt_render_frame* (the pinned-host form included) do what follows, with the same arguments and the same
 * argument checks as in mode 100; a failed call launches nothing.  The scene format's REFLECTIVE and REFRACTIVE materials,
 * which mode 100 shades as diffuse, are honoured deterministically: a camera looking at a mirror, a lidar's intensity behind a
 * window, a probe inside glass, a still of a .crtscene with its reflections and refraction.
 * - Segment 0 is the record (crt_shade_rays*) or the pixel-centre camera ray (frames).  It is traced exactly as crt_shade_rays
 *   traces it in mode 100 -- prescaled by 2^e, the same NaN / empty-interval rules, the same closest-hit traversal -- and the
 *   outputs t, uv, inst, prim, normal and albedo are those of its hit, as in mode 100.
 * - A record carries a throughput T = (1, 1, 1) and a turn count k = 0.  At the end of a segment:
 *     . miss: the colour is the miss colour if k == 0, else fmaf(T.c, miss.c, 0) per channel; the record ends;
 *     . REFLECTIVE (type 2): if k == max_bounces the colour is (0, 0, 0) and the record ends -- mode 200 cuts a chain the same
 *       way.  Otherwise T *= albedo (the texture's where the material has one), the next segment starts at the hit point moved
 *       1e-3 along the shading normal, in the normalised mirror direction, over (0, 10000), and k += 1;
 *     . REFRACTIVE (type 3): the same cut.  Otherwise Snell's direction with eta = 1 / ior entering and ior leaving, from the
 *       point moved 1e-3 to the far side; on total internal reflection the mirror direction from the near side.  T is unchanged,
 *       k += 1.  There is no Fresnel split and no branching: glass refracts or, past the critical angle, mirrors;
 *     . CONSTANT (type 4): the colour is fmaf(T.c, albedo.c, 0), also at k == 0, as in mode 200; the record ends;
 *     . anything else (DIFFUSE, an invalid type, a triangle without a material): mode 100's shading at this surface -- one
 *       any-hit shadow ray per light with a positive cosine, in light order, from the point moved 1e-3 along the normal over
 *       (0, distance), the frames' fmaf sequence, the options "phong_ks" and "phong_exponent".  Phong's view vector is minus this
 *       segment's direction: the record's direction as written for segment 0, the unit turn direction afterwards.  With L
 *       the sum, the colour is L itself if k == 0, else fmaf(T.c, L.c, 0); the record ends.
 *   These are the functions and the fmaf placement of the mode-200 path (crt_path_rays*) along the specular chain and of mode
 *   100 at its end.  So a record that meets no mirror and no glass gives mode 100's bits in every output, and with phong_ks =
 *   0 a record whose chain has k turns gives, at max_bounces = B, the rgb of crt_path_rays at one sample with max_bounces =
 *   min(B, k), bit for bit (tests/test_whitted.py).
 * - Options: "max_bounces" (0..64, default 3) also limits the turns of mode 150.  "spp" and "seed" are not read: there are no
 *   samples and no random numbers.
 * - Scale: segment 0 is scale-free as in mode 100 (any direction magnitude, the interval the record gives).  The bias 1e-3 and
 *   the interval (0, 10000) of later segments are absolute lengths, as in mode 200: mode 150 is not scale-free.  Snell's cosine
 *   and the mirror formula assume a unit direction on segment 0: a caller who wants the frames' semantics passes one.
 * - Frames: crt_render_frame* in mode 150 is the pixel-centre camera rays (crt_camera_rays, CRT_SAMPLE_CENTRE), this query over
 *   them and the frames' quantisation.  rgb_f32 is bit for bit crt_shade_rays of crt_camera_rays; rgba8 is its UNORM8; hit_t
 *   (10000 on a miss), hit_inst and hit_prim are those of the camera ray's own hit.  Such a frame leaves the launch orders
 *   and their cost state as it found them, and needs width x height <= 2^28 (CRT_EINVAL otherwise).  Accumulation ignores the
 *   mode, as it ignores mode 100; crt_frame_guides, the denoiser and the temporal passes work on such a frame as on any other.
 * - Not available (CRT_EINVAL, the message names the mode, nothing is launched): the tile entries (crt_render_tiles_device),
 *   the batch entries (crt_render_frames_batch_device, crt_render_tiles_batch_device) and crt_render_frame_distributed.
 * - stats: rays_primary = n (frames: the pixels); with crt_set_counting(ctx, 1) rays_primary is the exact number of closest-hit
 *   rays, records plus turns, rays_shadow the shadow rays, nodes_visited / tris_tested all traversals together.
 * - Pending refits are applied first.  Results do not depend on the order of the records, on scheduling, on the option
 *   "path_pass_paths" (a launch covers at most that many records: a larger buffer runs as several) or on inner_min,
 *   inner_min_any and stack_entries. */

/* ---- ambient occlusion (CRT_MODE_AMBIENT, 120): sky visibility per hit.  No function of its own: in mode 120 crt_shade_rays*
 * and crt_render_frame* (the pinned-host form included) do what follows, with the same arguments and the same argument checks
 * as in mode 100; a failed call launches nothing.  The result is the cosine-weighted share v of the hemisphere over a surface
 * point that is free of geometry within a radius -- ambient occlusion, the sky-view factor, accessibility: the contact shadows
 * of a still, a training target beside signed distance and occupancy, the visibility term of a sky-lit lidar return or probe --
 * estimated with K any-hit rays whose directions are drawn in registers: no ray buffer is written and no byte per ray read.
 * Options (crt_set_option; a value out of range -> CRT_EINVAL):
 *     "ao_samples"  K, 1..4096, default 16;
 *     "ao_radius"   0..1000000: the reach R of the occlusion rays in thousandths of the diagonal of the scene's bounding box,
 *                   so that it does not depend on the unit of length; default 0 = unbounded, R = 10000 (the interval of a
 *                   mode-200 bounce ray).  For a value v > 0, R = ((float)v / 1000.0f) * D with D = sqrtf((dx*dx + dy*dy) +
 *                   dz*dz), every operation rounded to float32 on its own (no fused multiply-add), where the box is that of node
 *                   0 of the binary tree as crt_bvh_export reports it at the time of the call (after a refit or a rebuild: the
 *                   new one): dx = fmaxf(nodes[0].lx1, nodes[0].rx1) - fminf(nodes[0].lx0, nodes[0].rx0), dy and dz likewise
 *                   from ly0 / ly1 / ry0 / ry1 and lz0 / lz1 / rz0 / rz1; a scene without triangles has D = 0;
 *     "ao_sky"      0/1, default 0: which colour step 5 gives;
 *     "seed"        the seed of mode 200 is read.  "spp" and "max_bounces" are not.
 * One record `id` (crt_shade_rays*: the index in the buffer; frames: the pixel-centre camera ray of pixel id = py * width + px):
 * 1. Closest hit: exactly that of crt_trace_rays.  t, uv, inst, prim, normal and albedo are mode 100's, bit for bit.  A miss,
 *    and a record that is not traced (NaN, empty interval), gives the miss colour, as in every mode, and ends.
 * 2. Surface: position P, shading normal N flipped to face the ray, and albedo as in mode 100; every material is treated as
 *    diffuse, as mode 100 treats it.  Po = P moved 1e-3 along N (fmaf(N.c, 1e-3f, P.c)).
 * 3. Occlusion samples s = 0 .. K - 1: with the hash h() and the generator next() of mode 200 (a PCG permutation of 32 bits;
 *    next(st): st = h(st), the value (st >> 8) * 2^-24),
 *        st = h(h(h(id ^ h(s + h(seed))))),  u1 = next(st),  u2 = next(st),  d = the cosine-weighted direction about N for
 *    (u1, u2) -- the two numbers the mode-200 path of (id, s, seed) draws for its first bounce, right after the two its pixel
 *    jitter takes, and the direction that path takes at a diffuse first hit with this normal.  One any-hit traversal from Po
 *    along d over (0, R), as crt_occluded_rays answers the record {Po, 0, d, R}.  `visible` counts the samples not occluded.
 * 4. Visibility: v = (float)((double)visible / (double)K).  `visible` is an integer: nothing depends on the order of the samples.
 * 5. Colour.  "ao_sky" = 0: rgb = (v, v, v).  "ao_sky" = 1: with `direct` mode 100's rgb at this hit (one shadow ray per light
 *    with a positive cosine, in light order, the options "phong_ks" / "phong_exponent" included), rgb.c = fmaf(albedo.c *
 *    miss.c, v, direct.c): point lights plus a sky of the miss colour.  With a black miss colour that is mode 100 bit for bit.
 * So with no lights, every material DIFFUSE and white, a white miss colour and "ao_radius" = 0, rgb is bit for bit that of
 * crt_path_rays with n_samples = K, max_bounces = 1 and the same seed: each of its samples is 1 or 0 as its first bounce ray
 * escapes or not (tests/test_occlusion_mode.py).
 * - Scale: the closest hit is scale-free as in mode 100.  The bias 1e-3 is an absolute length, as in modes 100 and 200, and so
 *   is the unbounded reach of 10000; a radius given by "ao_radius" follows the scene.
 * - Frames: crt_render_frame* in mode 120 is the pixel-centre camera rays (crt_camera_rays, CRT_SAMPLE_CENTRE), this query over
 *   them and the frames' quantisation, exactly as in mode 150: rgb_f32 is bit for bit crt_shade_rays of crt_camera_rays, rgba8
 *   its UNORM8, hit_t (10000 on a miss), hit_inst and hit_prim those of the camera ray's hit.  Such a frame leaves the launch
 *   orders and their cost state as it found them, needs width x height <= 2^28 (CRT_EINVAL otherwise), and neither reads nor
 *   changes the accumulation.
 * - Not available (CRT_EINVAL, the message names the mode, nothing is launched): the tile entries (crt_render_tiles_device),
 *   the batch entries (crt_render_frames_batch_device, crt_render_tiles_batch_device) and crt_render_frame_distributed.
 * - stats: rays_primary = n (frames: the pixels); with crt_set_counting(ctx, 1) rays_shadow is the exact number of any-hit rays,
 *   occlusion samples (K per hit) plus, with "ao_sky", the shadow rays; nodes_visited / tris_tested all traversals together.
 * - Pending refits are applied first.  Results do not depend on the order in which records are scheduled, on inner_min,
 *   inner_min_any or stack_entries; they do depend on a record's index, which is its id. */

/* ---- path-traced ray queries: mode-200 radiance for caller-supplied rays (the sample-indexing contract crt_shade_rays'
 * refusal of mode 200 asks for).  Global illumination for sensors that are not a pinhole -- fisheye and equirectangular
 * cameras, calibrated lenses, light and irradiance probes, lidar returns with interreflection, light fields -- without
 * rendering pinhole frames and resampling them.
 * - Records: the 8-float records of crt_trace_rays, with the same NaN / empty-interval / zero-direction rules and the same
 *   direction-magnitude contract.  The first segment is traced prescaled by 2^e, exactly as crt_trace_rays traces it, over the
 *   record's own (tmin, tmax): t / uv / inst / prim are crt_trace_rays' outputs for that record bit for bit and do not depend
 *   on the sample.  Each output is optional; at least one of rgb, sums, t, uv, inst, prim must be non-NULL.
 * - What a path is: each record is traced as n_samples independent paths, samples first_sample .. first_sample + n_samples - 1.
 *   Each is the frames' mode-200 path ("Path tracing") from its first segment on.  Per segment: a miss
 *   adds throughput x miss colour; CONSTANT emits and stops; REFLECTIVE and REFRACTIVE continue as in the frames (total
 *   internal reflection and the +-1e-3 bias included); DIFFUSE gathers direct light with one shadow ray per light that has a
 *   positive cosine, in light order, then takes the cosine-weighted bounce; textures are honoured; every fmaf stays where the
 *   frames have it.  Later segments run over (0, 10000) with the frames' cull bound.  max_bounces, seed, the miss colour and
 *   the textures come from the context.  The option spp and the context's shading mode are not read: the call path-traces in
 *   whatever mode the context is in and leaves the mode alone.
 * - What the shading sees: the record's own origin and direction and the unscaled t; nothing is normalised, as in
 *   crt_shade_rays.  Snell's cosine and the mirror formula assume unit directions: a caller who wants the frames' semantics
 *   passes them.  A miss or an untraced record is one segment whose radiance is the miss colour.
 * - Sample indexing: the path id of record i is ids[i], or i when ids is NULL.  The path of (id, sample s) starts its RNG at
 *   hash(id ^ hash(s + hash(seed))), the frames' start for pixel `id`, then takes two draws it does not use (in a frame: the
 *   pixel jitter), so that its first used draw is the frames' first bounce draw.  Hence:
 *     . a record that holds a frame's jittered camera ray for pixel p and sample s (id = py * width + px, origin = the camera
 *       position, tmin = 0.001, tmax = 10000) gives that path's radiance bit for bit;
 *     . results do not depend on the order of the records when their ids travel with them; the same ray with another id is
 *       another, equally valid, sample;
 *     . a caller who wants jitter from the same stream computes it on the host (Python: path_jitter).
 * - Sums and the mean: per record the samples' radiances are added in sample order into three float64 sums, as the frames add
 *   theirs.  Without sums, rgb = (float)(S / n_samples).  With sums (n x 3 float64, in / out): the stored values are the
 *   starting point when first_sample > 0, zero is when first_sample == 0 (the buffer is then not read); the new sums are
 *   written back and rgb = (float)(S / (first_sample + n_samples)).  So K calls of S samples equal one call of K * S samples
 *   bit for bit, and a caller may hand over different rays per call (its own jitter): the frames' accumulation with the sums
 *   owned by the caller and the context stateless.
 * - Passes: one launch covers at most the option "path_pass_paths" (record, sample) pairs; more run as several passes over
 *   sample ranges, with no effect on any result.
 * - Pending refits are applied first.  Camera, mode, accumulation sums, launch orders and frame outputs are untouched: a frame
 *   rendered after any number of calls equals the frame rendered without them, accumulating mode-200 runs included.  Inert
 *   triangles are never hit and never occlude; the boundary-ray limit of the ray queries applies unchanged.  Results do not
 *   depend on scheduling, on the pass split or on the options inner_min, inner_min_any and stack_entries.
 * - n = 0 returns CRT_OK and launches nothing.  CRT_ESTATE without a scene.  CRT_EINVAL for a NULL ctx, NULL rays with n > 0,
 *   n_samples == 0, first_sample + n_samples > 2^24 (the frames' limit), all six outputs NULL, or a misaligned device pointer
 *   (rays 16-byte; sums and uv 8-byte; everything else, ids included, 4-byte).  These checks come before the refit: a failed
 *   call launches nothing.
 * - stats (may be NULL): kernel_ms covers all kernels of the call; rays_primary = n * n_samples.  With crt_set_counting(ctx, 1)
 *   rays_primary is the exact number of closest-hit rays, bounce rays included, and rays_shadow / nodes_visited / tris_tested
 *   are counted as the frames count them: for a buffer of a frame's sample-0 camera rays they are the oracle's statistics of
 *   that 1-spp frame.
 * *_device: device pointers, asynchronous on the context's stream (crt_set_stream) unless stats != NULL.  Host variant:
 * synchronous, staged through the context's query staging buffer. */
int crt_path_rays_device(crt_ctx* ctx, uint32_t n, const void* d_rays, const void* d_ids, uint32_t first_sample, uint32_t n_samples,
                         void* d_rgb, void* d_sums, void* d_t, void* d_uv, void* d_inst, void* d_prim, crt_frame_stats* stats);
int crt_path_rays(crt_ctx* ctx, uint32_t n, const float* rays, const uint32_t* ids, uint32_t first_sample, uint32_t n_samples,
                  float* rgb, double* sums, float* t, float* uv, uint32_t* inst, uint32_t* prim, crt_frame_stats* stats);

/* ---- camera rays: the frames' own camera rays as ray records (what a DXR rayGen shader computes from DispatchRaysIndex; the
 * "record that holds a frame's camera ray" of crt_shade_rays* and crt_path_rays* without restating the ray generation).
 * - Writes width * height records of 8 floats (the crt_trace_rays layout) in row-major pixel order, record py * width + px:
 *   origin = the context's camera position (crt_set_camera), tmin = 0.001, direction = the frames' rayGen direction for that
 *   pixel, tmax = 10000.
 * - sample == CRT_SAMPLE_CENTRE: the jitter (0.5, 0.5), the rays of modes 0..100.  Otherwise (sample < 2^24): the two draws a
 *   mode-200 frame takes for pixel id py * width + px and frame sample index `sample` with the context's seed (option "seed";
 *   Python: path_jitter(ids, sample, seed)).  The mode is not read.
 * - Bit for bit the ray the frame kernels trace: the kernel calls the frames' ray generation and hash chain, nothing is
 *   restated.  So crt_shade_rays on the CRT_SAMPLE_CENTRE records gives a frame's rgb_f32 and hit_t in modes 0..100, and
 *   crt_path_rays with first_sample = k, n_samples = 1 on the records of sample k, chained through one sums buffer for k = 0 ..
 *   spp - 1, gives the mode-200 frame of spp samples.
 * - Needs no scene.  Camera, mode, accumulation sums, launch orders and frame outputs are untouched.
 * - CRT_EINVAL for a NULL ctx, a NULL buffer, width or height 0, width * height > 2^28, sample in [2^24, 0xFFFFFFFE], or a
 *   device pointer that is not 16-byte aligned; nothing is launched then.
 * - stats (may be NULL): kernel_ms, total_ms, rays_primary = width * height (rays generated; nothing is traced).
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variant: synchronous, staged. */
#define CRT_SAMPLE_CENTRE 0xFFFFFFFFu
int crt_camera_rays_device(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t sample, void* d_rays, crt_frame_stats* stats);
int crt_camera_rays(crt_ctx* ctx, uint32_t width, uint32_t height, uint32_t sample, float* rays, crt_frame_stats* stats);

/* ---- frame guide buffers: per pixel the shading normal (3 floats), the albedo (3 floats) and t of the pixel-centre camera
 * ray: the feature buffers an image-space denoiser is guided by (below), in the layout of rgb_f32 / hit_t.
 * - Exactly what crt_shade_rays returns as normal, albedo and t for the CRT_SAMPLE_CENTRE records of crt_camera_rays, bit for
 *   bit: a miss gives normal = albedo = (0, 0, 0) and t = 10000.  Each output is optional; not all three may be NULL.
 * - Works in every shading mode, mode 200 included (the mode is not read: the surface evaluation does not depend on it).  A
 *   separate pass over the camera rays: the frame kernels are not involved and a frame costs what it cost before.
 * - The queries' common rules: pending refits are applied first; CRT_ESTATE without a scene; camera, mode, accumulation sums,
 *   launch orders and frame outputs are untouched -- an accumulating mode-200 run goes on as if the call had not happened.
 * - CRT_EINVAL for a NULL ctx, width or height 0, width * height > 2^28, all three outputs NULL, or a device pointer that is
 *   not 4-byte aligned.  These checks come before the refit: a failed call launches nothing.
 * - stats (may be NULL): kernel_ms = the camera-ray kernel and the shaded query together, rays_primary = width * height; with
 *   crt_set_counting(ctx, 1) nodes_visited / tris_tested as crt_shade_rays counts them.
 * - Temporary memory: 32 B per pixel (the records) in the context's query arena of the stream.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variant: synchronous, staged. */
int crt_frame_guides_device(crt_ctx* ctx, uint32_t width, uint32_t height, void* d_normal, void* d_albedo, void* d_t,
                            crt_frame_stats* stats);
int crt_frame_guides(crt_ctx* ctx, uint32_t width, uint32_t height, float* normal, float* albedo, float* t, crt_frame_stats* stats);

/* ---- denoiser: the edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) on row-major width x height
 * buffers: rgb, normal, albedo (3 floats per pixel) and t (1 float per pixel), the layouts of rgb_f32 and of crt_frame_guides.
 * A pure image-space filter: no scene is needed and any colour / guide buffers of that layout will do.
 * - Live pixels: a pixel is live when all 10 of its input values are finite, its normal has a non-zero component and t > 0.
 *   A pixel that is not live (a miss, a NaN firefly, a hole the caller cut) is copied from rgb to out bit for bit and is never
 *   a tap of another pixel.
 * - Demodulation: a = demodulate ? max(albedo, 1e-3) per channel : 1, and c_0 = rgb / a (texture detail is divided out,
 *   filtered irradiance is multiplied back).  rgb / a must stay finite.
 * - Pass i = 0 .. iterations - 1: stride s = 2^i, sigma_c,i = sigma_color 2^-i.  For a live centre p the taps are q = p +
 *   s (dx, dy), dx, dy in -2 .. 2; only taps inside the image and live are used.
 *     e = |c_i(p) - c_i(q)|^2 / sigma_c,i^2 + |n_p - n_q|^2 / sigma_normal^2 + (t_p - t_q)^2 / (sigma_depth t_p)^2
 *     w = h[dx + 2] h[dy + 2] exp(-e),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *     c_{i+1}(p) = sum w c_i(q) / sum w      (the centre tap has e = 0, w = 9/64: the divisor is positive)
 * - Output: out = c_N a.
 * - Arithmetic: float32 throughout.  There is no bit-for-bit contract against a CPU form, because exp has none.  What holds:
 *   the deviation from a float64 evaluation of the formulas above stays within 16 x that of a float32 evaluation on the host
 *   (metric |x - ref| / max(|ref|, 1e-3); tests/test_denoise.py); determinism -- no atomics, the same input gives the same
 *   bits; and the host form equals the device form bit for bit.
 * - Aliasing: d_out may equal d_rgb (in place); no other two buffers may overlap.
 * - params == NULL means the defaults.  CRT_EINVAL for iterations outside 1..8; a sigma that is <= 0 or NaN (+inf is allowed
 *   and switches its term off); demodulate other than 0 / 1; width or height 0; width * height > 2^28; a NULL context or
 *   buffer; a device pointer that is not 4-byte aligned.  A failed call launches nothing and leaves out untouched.
 * - stats (may be NULL): kernel_ms = all kernels of the call, total_ms; every count is zero.
 * - Scratch is context-owned (the query arena of the stream), grows on demand and is freed by crt_destroy: 48 B per pixel --
 *   the guide plane {n, t} and two colour planes {c, live}, 16 B each.  CRT_ENOMEM when it cannot be had, nothing launched.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variant: synchronous, staged. */
typedef struct crt_denoise_params {
    uint32_t iterations;  /* 1..8, default 5: pass i samples at stride 2^i */
    float sigma_color;    /* default 4.0; halved every pass */
    float sigma_normal;   /* default 0.3 */
    float sigma_depth;    /* default 0.05, relative to the centre pixel's t */
    uint32_t demodulate;  /* default 1: filter rgb / albedo, multiply back at the end */
} crt_denoise_params;
int crt_denoise_device(crt_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgb, const void* d_normal, const void* d_albedo,
                       const void* d_t, void* d_out, const crt_denoise_params* params /* NULL = defaults */, crt_frame_stats* stats);
int crt_denoise(crt_ctx* ctx, uint32_t width, uint32_t height, const float* rgb, const float* normal, const float* albedo,
                const float* t, float* out, const crt_denoise_params* params, crt_frame_stats* stats);

/* ---- temporal reprojection: a path-traced frame blended with the history of earlier frames, carried across camera moves (the
 * first half of a production denoiser; crt_denoise is the second).  Buffers are row-major width x height: rgb, normal, albedo
 * (3 floats per pixel) and t (1 float per pixel) of the current frame, the layouts of rgb_f32 and of crt_frame_guides.
 * - A history record is 8 floats (32 B, 16-byte aligned) per pixel, row-major: {c.r, c.g, c.b, len, n.x, n.y, n.z, t}.  The
 *   caller owns two such buffers and swaps them every frame: hist_next of one call is hist_prev of the next, together with
 *   that call's cam_cur as cam_prev.  The context keeps no state (the design of crt_path_rays' sums).
 * - Cameras: 12 floats {pos[3], rot3x3_rowmajor[9]}, the layout of the batch entry points; host pointers in both forms.  The
 *   rotation is taken as orthonormal.
 * - Pure image space: no scene is needed; the context's camera and mode are not read; accumulation sums, launch orders and
 *   frame outputs are untouched.
 * - The contract, per pixel p = (px, py).  All arithmetic is float32; fmaf appears only where written; / is correctly rounded;
 *   dot(x, y) = fmaf(x.z, y.z, fmaf(x.y, y.y, x.x * y.x)); w and h are the sizes as floats; dir(rot, x, y) is the direction of
 *   the frames' pixel-centre camera ray of pixel (x, y) (crt_camera_rays with CRT_SAMPLE_CENTRE) for that rotation.
 *    1. Live: rgb, normal and t are finite, the normal has a non-zero component and t > 0; when demodulating, albedo is finite
 *       too (crt_denoise's rule).
 *    2. a = demodulate ? max(albedo, 1e-3) per channel : 1;  c = rgb / a.  albedo may be NULL only when demodulate == 0.
 *    3. A pixel that is not live: out = rgb bit for bit, hist_next = {rgb bits, 0, n, t}.  A record whose len is not > 0, or
 *       that holds any non-finite value, is never a tap.
 *    4. d = dir(rot_cur, px, py);  P = o_cur + d * t per component (a product, then a sum).
 *    5. v = P - o_prev;  pc = (dot(col0(R_prev), v), dot(col1(R_prev), v), dot(col2(R_prev), v)).
 *    6. s = -pc.z; no history unless s > 0.
 *         fx = ((pc.x / s) / (w / h) + 1) * 0.5 * w - 0.5        fy = (1 - pc.y / s) * 0.5 * h - 0.5
 *       (evaluated left to right); no history unless fx > -1 && fx < w && fy > -1 && fy < h (a NaN fails).
 *    7. When the 12 floats of cam_prev equal those of cam_cur bitwise: fx = px, fy = py exactly, steps 5 and 6 are skipped.
 *    8. x0 = floor(fx), wx = fx - x0, likewise y0, wy.  Taps k = 0..3: (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
 *       with b_k = (1 - wx)(1 - wy), wx (1 - wy), (1 - wx) wy, wx wy.
 *    9. A tap q is valid when it is inside the image, its record of hist_prev is usable (3),
 *       |dot(n_p, Pq - P)| <= depth_tolerance * t_p with Pq = o_prev + dir(rot_prev, qx, qy) * t_q, and
 *       dot(n_p, n_q) >= normal_threshold.
 *   10. Over the valid taps in the order k = 0..3, each sum starting at 0:  W = sum b_k,  S = sum b_k * c_q (a product, then a
 *       sum),  SL = sum b_k * len_q.  No history unless W >= 0.01.  hc = S / W,  L = SL / W.
 *   11. With history: a_t = max(alpha, 1 / (L + 1)), c_out = fmaf(a_t, c - hc, hc), len_out = min(L + 1, max_history).
 *       Without (also: hist_prev == NULL): c_out = c, len_out = 1.
 *   12. hist_next = {c_out, len_out, n_p, t_p};  out = c_out * a.
 *   alpha = 0 is the plain running mean of up to max_history frames; with alpha > 0 the mean turns into an exponential one
 *   once 1 / (len + 1) falls below alpha.  tests/temporal_reference.c restates these steps in C; the kernel equals it bit for bit.
 * - Object motion is not seen by this call: after crt_update_vertices, crt_set_mesh_transform, crt_refit or crt_rebuild a surface
 *   that slid within its own plane keeps stale history (the plane-distance and normal tests cannot see it) and one that moved
 *   along its normal loses it.  Use crt_temporal_accumulate_motion* with the previous points of crt_frame_motion* /
 *   crt_previous_points* (below, "motion"), or drop the history by passing d_hist_prev = NULL.  Variance estimation and second
 *   moments (SVGF) are crt_temporal_variance* (below, "variance").
 * - Aliasing: d_out may equal d_rgb; d_hist_next must not overlap d_hist_prev; no other two buffers may overlap.  d_out may be
 *   NULL (only the history is wanted).
 * - params == NULL means the defaults.  CRT_EINVAL for a NULL context or camera; a NULL rgb, normal, t or hist_next; a NULL
 *   albedo while demodulating; width or height 0; width * height > 2^28; alpha outside [0, 1] or NaN; depth_tolerance not > 0;
 *   normal_threshold NaN; max_history outside 1..2^24; demodulate other than 0 / 1; a misaligned device pointer (history:
 *   16-byte, the rest: 4-byte).  A failed call launches nothing and writes nothing.
 * - stats (may be NULL): kernel_ms, total_ms; every count is zero.
 * - No scratch memory: one kernel, one thread per pixel, no atomics -- the same input gives the same bits.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variant: synchronous, staged. */
typedef struct crt_temporal_params {
    float alpha;            /* default 0.1: least weight of the new frame; 0 = plain running mean up to max_history */
    float depth_tolerance;  /* default 0.01: plane distance allowed, relative to the centre pixel's t */
    float normal_threshold; /* default 0.9: least dot(n_p, n_q) */
    uint32_t max_history;   /* default 64, 1..2^24: cap of the history length */
    uint32_t demodulate;    /* default 1: history holds rgb / max(albedo, 1e-3) */
} crt_temporal_params;
int crt_temporal_accumulate_device(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12], const float cam_prev[12],
                                   const void* d_rgb, const void* d_normal, const void* d_albedo, const void* d_t,
                                   const void* d_hist_prev /* NULL = no history */, void* d_hist_next, void* d_out /* may be NULL */,
                                   const crt_temporal_params* params /* NULL = defaults */, crt_frame_stats* stats);
int crt_temporal_accumulate(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12], const float cam_prev[12],
                            const float* rgb, const float* normal, const float* albedo, const float* t, const float* hist_prev,
                            float* hist_next, float* out, const crt_temporal_params* params, crt_frame_stats* stats);

/* ---- point queries: closest surface point, hit counts, occupancy (no reference counterpart; the set of Open3D's
 * RaycastingScene: compute_closest_points / compute_distance / compute_signed_distance / compute_occupancy /
 * count_intersections).  SDF and occupancy training data, collision margins, snapping a point to the surface.
 * - Point record: 4 floats (16 B) {x, y, z, rmax}; the buffer holds n records, contiguous.
 * - Closest point (crt_closest_points*): over every triangle's leaf-ordered record {v0, e1, e2} as traced (a = v0, ab = e1,
 *   ac = e2), the triangle of smallest computed d2 among those with d2 <= rmax * rmax; equal d2 goes to the lower global
 *   triangle id (upload ordinal), the frames' tie rule.  Outputs, each optional, not all NULL: dist = sqrtf(d2), point (3 floats,
 *   the closest point), uv (2 floats: u = weight of v1, v = weight of v2, as in crt_trace_rays), inst, prim.  A miss (no
 *   triangle within rmax, a record with a NaN, rmax < 0, an empty scene) reports dist = rmax, point = the query point, uv = 0,
 *   inst = prim = CRT_MISS.  rmax = +inf is allowed.
 * - Operation order (float, fused multiply-adds only where fmaf is written, / and sqrtf correctly rounded; dot(x, y) =
 *   fmaf(x.z, y.z, fmaf(x.y, y.y, x.x * y.x))): Ericson's region method (Real-Time Collision Detection 5.1.5) on (a, ab, ac):
 *     ap = p - a; bp = ap - ab; cp = ap - ac;  d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp),
 *     d5 = dot(ab, cp), d6 = dot(ac, cp)  (each vector difference per component)
 *     d1 <= 0 && d2 <= 0 -> (u, v) = (0, 0);  else d3 >= 0 && d4 <= d3 -> (1, 0);
 *     else vc = d1*d4 - d3*d2; vc <= 0 && d1 >= 0 && d3 <= 0 && d1 - d3 > 0 -> (d1 / (d1 - d3), 0);
 *     else d6 >= 0 && d5 <= d6 -> (0, 1);
 *     else vb = d5*d2 - d1*d6; vb <= 0 && d2 >= 0 && d6 <= 0 && d2 - d6 > 0 -> (0, d2 / (d2 - d6));
 *     else va = d3*d6 - d5*d4, e = d4 - d3, f = d5 - d6; va <= 0 && e >= 0 && f >= 0 && e + f > 0 -> w = e / (e + f), (1 - w, w);
 *     else s = (va + vb) + vc; va > 0 && vb > 0 && vc > 0 && s < +inf -> (vb / s, vc / s) (the face), and when the triangle
 *     is a sliver, s <= 2^-10 * (dot(ab, ab) * dot(ac, ac)), the nearer of that point and the edge candidates below (face
 *     first on equal d2);
 *     else (degenerate triangles, rounding at a region border) the nearest of the three edges: per edge (base, e) in the order
 *     (a, ab), (a, ac), (b, ac - ab) with base offset g = ap, ap, bp: t = ee > 0 ? min(max(dot(g, e) / ee, 0), 1) : 0,
 *     ee = dot(e, e), giving (t, 0), (0, t), (1 - t, t); each candidate's d2 as below, the first smallest one wins.
 *   Then r = fmaf(-v, ac, fmaf(-u, ab, ap)) per component and d2 = dot(r, r); point = fmaf(v, ac, fmaf(u, ab, a)).  Every
 *   division has a positive divisor, so no triangle -- zero area, collinear, all three vertices equal -- yields a NaN.
 * - Hit count (crt_count_hits*): ray records of crt_trace_rays with their NaN and empty-interval rules and their direction
 *   magnitude contract (prescaled the same way; counts do not depend on |d|); the number of triangles that the ray queries'
 *   Moeller-Trumbore test accepts with tmin < t < tmax, every one of them (no early exit).
 *   The "boundary rays" limit of the ray queries applies unchanged.
 * - Occupancy (crt_occupancy*): one byte per point, 1 when at least two of the hit counts of the rays {p, tmin = 0,
 *   CRT_OCCUPANCY_DIRk, tmax = +inf}, k = 0..2, are odd.  rmax is ignored.  The directions lie at least 16 degrees from
 *   every axis plane and every cube diagonal, so that grid-sampled points over axis-aligned meshes do not hit edges and
 *   vertices systematically.  Meaningful for closed meshes; undefined for points on a surface; for open geometry it is
 *   the majority of three crossing parities, nothing more.  A point with a NaN coordinate is outside.
 * - Results do not depend on the tree (host SAH, gpu_build LBVH or PLOC, refitted or rebuilt), on the order of the records
 *   or on scheduling: the closest-point search prunes a box only when no triangle in it can produce a computed d2 <= the
 *   best so far (the margin holds at any offset from the origin).
 *   Inert triangles (non-finite vertices, above) are never the closest triangle and are never counted, over any tree.
 * - Scene scale: vertices, points and rmax times 2^k give the same inst, prim, uv and occupancy, and dist and point times 2^k,
 *   bit for bit, while every intermediate stays a normal float.  The region tests multiply two dot products (vc = d1*d4 -
 *   d3*d2: fourth order in a length), so the closest point has the narrowest range of all queries: measured as for the ray
 *   queries (scene of extent 4, tests/test_scale_similarity.py) k = -28 .. 30; occupancy, three hit
 *   counts, -45 .. 42.  Outside it results change without an error; kernel and reference still agree bit for bit there.
 * - Common rules of the ray queries: pending refits are applied first; a query reads the tree and the triangle records,
 *   nothing else (camera, mode, accumulation sums, launch orders, frame outputs are untouched); n = 0 returns CRT_OK and
 *   launches nothing; CRT_ESTATE without a scene.  stats (may be NULL): kernel_ms, total_ms, rays_primary = records traced
 *   (n; 3n for occupancy), nodes_visited / tris_tested with crt_set_counting(ctx, 1), counted as the frames count them.
 * *_device: device pointers: points 16-byte, rays 16-byte, dist / point / inst / prim / count 4-byte, uv 8-byte aligned
 * (CRT_EINVAL otherwise); asynchronous on the context's stream unless stats != NULL.  Host forms: synchronous, staged. */
#define CRT_OCCUPANCY_DIR0 0x1.75de06p-1f, 0x1.2704acp-2f, 0x1.3d302ap-1f     /* ( 0.730209529,  0.288103759,  0.619508088) */
#define CRT_OCCUPANCY_DIR1 -0x1.137b5p-1f, 0x1.84aca6p-1f, -0x1.7728acp-2f    /* (-0.538050175,  0.759129703, -0.366366088) */
#define CRT_OCCUPANCY_DIR2 0x1.adef4p-2f, -0x1.69be36p-2f, -0x1.ac0a56p-1f    /* ( 0.419857979, -0.353264660, -0.836016357) */
int crt_closest_points_device(crt_ctx* ctx, uint32_t n, const void* d_points, void* d_dist, void* d_point, void* d_uv,
                              void* d_inst, void* d_prim, crt_frame_stats* stats);
int crt_closest_points(crt_ctx* ctx, uint32_t n, const float* points, float* dist, float* point, float* uv,
                       uint32_t* inst, uint32_t* prim, crt_frame_stats* stats);
int crt_count_hits_device(crt_ctx* ctx, uint32_t n, const void* d_rays, void* d_count, crt_frame_stats* stats);
int crt_count_hits(crt_ctx* ctx, uint32_t n, const float* rays, uint32_t* count, crt_frame_stats* stats);
int crt_occupancy_device(crt_ctx* ctx, uint32_t n, const void* d_points, void* d_inside, crt_frame_stats* stats);
int crt_occupancy(crt_ctx* ctx, uint32_t n, const float* points, uint8_t* inside, crt_frame_stats* stats);

/* ---- winding numbers: the inside test for open meshes and triangle soups (no reference counterpart; Jacobson, Kavan,
 * Sorkine-Hornung 2013, "Robust inside-outside segmentation using generalized winding numbers", evaluated over the tree as in
 * Barill, Dickson, Schmidt, Levin, Jacobson 2018, "Fast winding numbers for soups and clouds", first order).  The generalised
 * winding number w of a point is the sum of the signed solid angles of all triangles over 4 pi: 1 inside and 0 outside a closed
 * outward-oriented mesh, -1 inside a reversed one, 2 inside two nested shells, a smooth fraction near a hole.  w > 0.5 is the
 * inside test crt_occupancy cannot give for open geometry.
 * - Records: the point records of crt_closest_points, 4 floats {x, y, z, rmax}; rmax is ignored.  Output: one float per point.
 * - Per-triangle term h (half the signed solid angle; float, fused multiply-adds only where fmaf is written, / and sqrtf
 *   correctly rounded, dot as in the point queries), from the leaf-ordered record {v0, e1, e2} as traced and the point q:
 *     a = v0 - q; b = a + e1; c = a + e2  (per component)
 *     E = expo(the largest of the nine |components| of a, b, c), where expo(m) is the exponent frexpf gives (m = f 2^E, f in
 *       [0.5, 1)) and 0 when m is zero or not finite; a NaN component is never the largest
 *     a = ldexpf(a, -E), e1 = ldexpf(e1, -E), e2 = ldexpf(e2, -E) per component (exact: the triangle as seen from q, brought to
 *       unit size; the solid angle has no dimension);  b = a + e1; c = a + e2 again, from the scaled values
 *     n = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x);  det = dot(a, n)
 *       (the edge form of a . (b x c): its rounding error grows with the triangle's size, not with the cube of its distance)
 *     la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));  m = (la * lb) * lc
 *     den = ((m + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
 *     h = m == 0 ? 0 : crtAtan2(det, den)        (m == 0: the point is a vertex of the triangle -- after the scaling the largest
 *       of la, lb, lc is at least 0.5 and a length is zero only when its vector is below 2^-75 of that: the product of three
 *       lengths no longer underflows because the scene is small)
 *   Where a, b, c, e1, e2 and every product were normal floats without the scaling, h has the bits it would have without it.
 * - crtAtan2(y, x), the project's own arctangent (neither the device library's atan2f nor libm's: they differ):
 *     ay = |y|, ax = |x|; swap = ay > ax; mx = swap ? ay : ax; mn = swap ? ax : ay
 *     t = mn / mx; s = t * t; p = C6; p = fmaf(p, s, Ck) for k = 5 .. 0; r = fmaf(t, s * p, t)
 *     swap -> r = PI_2 - r;  x < 0 -> r = PI - r  (PI = 0x1.921fb6p+1f, PI_2 = 0x1.921fb6p+0f);  result y < 0 ? -r : r
 *     and r = 0 when y or x is a NaN, when both are zero, or when either is infinite.
 *   So y = +-0 gives +0 for x > 0 (a point in the triangle's plane outside the triangle) and +PI for x < 0 whichever the sign of
 *   the zero (in the plane inside the triangle: undefined on the surface, but the same bits from both sides); x = +-0 gives
 *   +-PI_2.  Absolute error against atan2 in float64: at most 2.95e-7 measured over the grid of tests/test_winding.py (the test
 *   asserts that figure plus one float32 ulp of pi, under the 2^-20 the error budget below needs).
 *   Triangles that contribute exactly zero: inert ones (a non-finite vertex makes det or den a NaN or an infinity) and those
 *   with the point at a vertex (held on every poisoned upload, refit, rebuild and heal by tests/test_nonfinite_vertices.py
 *   through tests/winding_checks.py: exact mode equals brute force over the records with the inert ones deleted).  The scaled products cannot overflow: every component is below 2 in magnitude.  What is left
 *   of the float range is the subtraction v0 - q and the sums a + e1, a + e2 themselves, which overflow only within a factor 2
 *   of FLT_MAX (E = 0 then, and the triangle contributes zero), and components 2^-126 and more below the largest, which the
 *   scaling rounds.  A record with a NaN coordinate gives w = 0.
 * - Sum: every contribution h, a triangle's or a cluster's, is added to a 64-bit integer as llrint((double)h * 2^36); the
 *   result is w = (float)((double)sum * 2^-36 / (2 pi)), 2 pi = 6.283185307179586.  Integer addition is associative: w does not
 *   depend on the order of the walk, of the records or on scheduling.  |h| <= pi < 2^38 / 2^36, so the sum cannot wrap below
 *   2^25 triangles; a cluster's h is clamped to +-4096 before the conversion (a NaN counts as 0).
 * - Moments (crt_winding_moments_export: n_nodes4 x 32 floats): per wide node, words 4k .. 4k+3 = {p~.x, p~.y, p~.z, r} and
 *   words 16+4k .. 16+4k+3 = {N~.x, N~.y, N~.z, 0} of child slot k.  For the triangles below the child, in float64 from the
 *   float32 records, without fused multiply-add, with n_i = 0.5 * (e1 x e2) (component order as n above) and
 *   A_i = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z):  N~ = sum n_i,  A = sum A_i,  P = sum A_i * (v0 + (e1 + e2) / 3.0),  p~ = P / A
 *   (the child's box centre 0.5f * (lo + hi) when A = 0), each rounded to float32 once.  A leaf's sums start at 0 and take its
 *   triangles in leaf order; a node's total starts at 0 and takes its four slots in order 0..3; an inner child's sums are its
 *   node's total.  Inert triangles are left out; CRT_BVH_EMPTY slots hold zeros.  r (float) over the child's decoded
 *   quantised box [lo, hi]: r = sqrtf((mx + my) + mz), m_a = max((p~_a - lo_a)^2, (hi_a - p~_a)^2): no triangle of the child
 *   is farther from p~.  (tests/winding_checks.py moments_f64 restates this paragraph in float64, per child slot straight over
 *   the triangles below it, and holds every exported table to it: N~ and p~ to one float32 rounding plus the summation error,
 *   r against the vertices; tests/test_winding_checks.py shows that it rejects a table that counts an inert triangle.)
 * - Walk: from the root, per non-empty child slot with d0 = p~ - q: E = expo(the largest |component| of d0), d = ldexpf(d0, -E)
 *   per component, d2 = dot(d, d) (in [0.25, 3) for a finite non-zero d0), br = beta * ldexpf(r, -E): when beta > 0 and
 *   d2 > br * br the child contributes h = ldexpf((0.5f * dot(N~, d)) / (d2 * sqrtf(d2)), -2 * E) and is not entered; else it is
 *   entered; a leaf adds every triangle's term.  The comparison is d0 . d0 > (beta r)^2 with both sides divided by 2^2E: it
 *   cannot overflow on the left, and where neither side left the normal range before it decides as before.  The dipole is
 *   0.5 N~ . d0 / |d0|^3 with the length taken out; h itself has no dimension.  beta <= 0 or NaN: exact -- no cluster is approximated and w is the sum over all triangles, the same bits over every
 *   tree (host SAH, LBVH, PLOC, refitted, rebuilt; tests/test_winding.py test_exact_mode_is_the_same_over_every_tree and
 *   test_far_from_origin, tests/test_deep_stacks.py on trees whose exact-mode walk holds up to 57 stack entries and through
 *   every move of depth4, tests/test_nonfinite_vertices.py on poisoned scenes).  beta = +inf is exact through the same comparison.  With a finite beta > 0
 *   the result depends on the tree (other clusters exist), not on any order.  beta = 2 keeps the error near 1e-2 at worst
 *   close to a cluster and far below it elsewhere (DESIGN.md section 5q has the measured figures).
 * - Unit of length: w does not depend on it.  Vertices and points times 2^k give the same bits of w in exact mode wherever the
 *   scaled vertices and points are themselves normal floats (asserted for k = -118 .. 120 on a scene of extent 4, all that scene
 *   can express; tests/test_scale_similarity.py).  With beta > 0 the moment table is the bound: N~ is an
 *   area in squared units, rounded to float32, and r a length.  The same bits hold while every non-zero component of N~ and
 *   each product N~_i d_i is a normal float (d_i is below 1 in magnitude) and while the builder forms the
 *   same tree; measured k = -57 .. 58 at beta = 2 and -58 .. 58 at beta = 8 over the host SAH tree of that scene, whose
 *   smallest leaf clusters have an area near 2^-9 (the host builder's tree itself changes above k = 58 and below k = -70).
 *   Outside that range clusters whose N~ has underflowed contribute too little: use exact mode or rescale.
 * - Common rules of the point queries: pending refits are applied first; n = 0 returns CRT_OK and launches nothing;
 *   CRT_ESTATE without a scene; CRT_EINVAL for a NULL context, a NULL or misaligned pointer (points 16-byte, w 4-byte).  The
 *   moment table (n_nodes4 x 128 bytes) is built by the first winding query or export after an upload, a refit or a rebuild;
 *   that build waits for the stream.  Otherwise the device form is asynchronous on the context's stream unless stats != NULL.
 *   stats: rays_primary = n; nodes_visited / tris_tested with crt_set_counting(ctx, 1): node records (each with its moment
 *   line) and triangle records fetched.  Frames, accumulation and launch orders are untouched. */
#define CRT_ATAN_C0 -0x1.5550f2p-2f   /* -0.33331659 */
#define CRT_ATAN_C1 0x1.98d61p-3f     /*  0.19962704 */
#define CRT_ATAN_C2 -0x1.1e3d8ap-3f   /* -0.13976581 */
#define CRT_ATAN_C3 0x1.912bfap-4f    /*  0.09794233 */
#define CRT_ATAN_C4 -0x1.d947fp-5f    /* -0.05777356 */
#define CRT_ATAN_C5 0x1.797d4p-6f     /*  0.02304012 */
#define CRT_ATAN_C6 -0x1.1d6f7ap-8f   /* -0.00435540 */
int crt_winding_numbers_device(crt_ctx* ctx, uint32_t n, const void* d_points, float beta, void* d_w, crt_frame_stats* stats);
int crt_winding_numbers(crt_ctx* ctx, uint32_t n, const float* points, float beta, float* w, crt_frame_stats* stats);
int crt_winding_moments_export(const crt_ctx* ctx, float* moments /* n_nodes4 (crt_bvh_info4) x 32 floats */);

/* ---- all-hits ray queries: every crossing of a ray, sorted by distance (Open3D's list_intersections, Embree's rtcIntersect with
 * an all-hits filter, the any-hit shader of DXR).  Wall thickness and chord lengths, layered depth images, inside / outside with
 * the evidence attached, multi-return sensor casts.
 * - Rays: the 8-float records of crt_trace_rays, with the same NaN / empty-interval / zero-direction rules and the same
 *   direction-magnitude contract (traced prescaled by 2^e).
 * - Which hits: exactly the triangles crt_count_hits counts for that record: every triangle the ray queries' Moeller-Trumbore
 *   test accepts with tmin < t < tmax, no early exit, no culling against a best t.  offsets[i + 1] - offsets[i] is the count
 *   crt_count_hits reports for record i, for every ray, always.
 * - Layout (CSR): offsets[0] = 0, offsets[i] = number of hits of rays 0 .. i-1, offsets[n] = the total; uint64 values below
 *   2^63 (a torch.int64 tensor can receive them).  The hits of ray i are records offsets[i] .. offsets[i+1]-1 of the four
 *   record arrays: t (float, reported as t' 2^-e like crt_trace_rays), uv (2 floats, u = weight of v1, v = weight of v2),
 *   inst, prim (uint32: mesh ordinal and triangle of that mesh).  Each may be NULL; all four NULL makes the call an
 *   offsets-only call.
 * - Order inside a ray: ascending prescaled t' compared as floats; records of equal t' (==, so -0 and +0 are equal) in
 *   ascending global triangle id (upload ordinal), the frames' and the closest-hit query's tie rule.  A triangle sits in one
 *   leaf, so the order is total.  For a ray with hits, record offsets[i] is bit for bit the closest hit crt_trace_rays
 *   reports (t, u, v, inst, prim), boundary rays excepted.
 * - Capacity: `capacity` is the number of records each non-NULL record array can hold (ignored when all four are NULL).  The
 *   offsets are always written.  The records are written only if offsets[n] <= capacity; otherwise no byte of the four arrays
 *   is touched.  The call returns CRT_OK in both cases (too small a buffer is an answer, not an error) and *total =
 *   offsets[n] when total != NULL: the caller compares, allocates and calls again.  The decision is made on the device (the
 *   fill and sort kernels read offsets[n] and leave when it exceeds the capacity they were given).
 * - Asynchrony: the device form is asynchronous on the context's stream when total == NULL && stats == NULL; with either
 *   given it synchronises.  The host form is synchronous and staged; it reads the total back once between the count and the
 *   fill, traverses once when the records do not fit (or none are wanted) and copies no record array out then.
 * - Independence: results do not depend on the tree (host SAH, gpu_build LBVH or PLOC, refitted, rebuilt), on the order of
 *   the records, on scheduling, or on inner_min / inner_min_any / stack_entries / list_short_max.  The "boundary rays" limit
 *   of the ray queries applies unchanged and is the only exception, as for crt_count_hits.
 *   Inert triangles (non-finite vertices, above) appear in no list, over any tree.
 * - Common rules of the queries: pending refits are applied first; camera, mode, accumulation sums, launch orders and frame
 *   outputs are untouched; n = 0 returns CRT_OK and launches nothing (the host form writes offsets[0] = 0 when offsets !=
 *   NULL, the device form looks at no buffer; *total = 0); CRT_ESTATE without a scene; CRT_EINVAL for a NULL ctx, for NULL rays
 *   or offsets with n > 0, and for misaligned device pointers (rays 16-byte, offsets 8-byte, uv 8-byte, t / inst / prim
 *   4-byte).  A failed call launches nothing: these checks come before pending refits are applied.
 * - How: two traversals.  The hit count into a context-owned buffer, an exclusive sum into the offsets, the same traversal
 *   again writing each accepted hit (t', triangle record) into its ray's segment, a sort of every segment (one lane per ray
 *   up to option "list_short_max" records, default 24, speed only; one wavefront per longer ray) and a resolve pass that
 *   re-runs the triangle test for u, v as the closest-hit query does at retirement.
 * - stats: kernel_ms = all kernels of the call (count, scan, fill, sort; the host form's figure spans its read-back too),
 *   rays_primary = n.  With crt_set_counting(ctx, 1), nodes_visited / tris_tested are the records fetched by both traversals:
 *   exactly twice what crt_count_hits reports for the same buffer when the records are written, exactly once when they are not
 *   (offsets-only call, total above capacity, total = 0 in the host form).  The triangle records re-read by the sort's tie
 *   rule and by the resolve pass are not counted.
 * - Temporary memory is context-owned and grows on demand: n uint32 counts plus the scan's tile sums, per stream in use.  The
 *   device form adds 4 B x capacity for each of t and prim the caller did not supply while asking for another array (the sort
 *   keys live in those two arrays), allocated before anything is launched; CRT_ENOMEM if that fails, with nothing launched. */
int crt_list_hits_device(crt_ctx* ctx, uint32_t n, const void* d_rays, void* d_offsets /* (n + 1) x uint64 */, uint64_t capacity,
                         void* d_t, void* d_uv, void* d_inst, void* d_prim, uint64_t* total /* host, may be NULL */,
                         crt_frame_stats* stats);
int crt_list_hits(crt_ctx* ctx, uint32_t n, const float* rays, uint64_t* offsets, uint64_t capacity, float* t, float* uv,
                  uint32_t* inst, uint32_t* prim, uint64_t* total, crt_frame_stats* stats);

/* ---- dynamic geometry (DXR: acceleration-structure updates and D3D12_RAYTRACING_INSTANCE_DESC::Transform, which the reference
 * fills with the identity for every mesh, R/DXRTRenderer.cpp:690-704).  Opt-in: crt_set_option(ctx, "dynamic", 1) before
 * crt_upload_scene / crt_upload_scene_from; only then does the upload keep what a refit needs in HBM (the meshes' rest and world
 * vertices and normals, indices, the binary tree, its per-level node lists, room for a wide tree of one node per binary inner
 * node).  A context that never sets the option behaves, allocates and performs as without it.
 * - Each mesh has rest vertices / normals (those uploaded, or the last ones given to crt_update_vertices*) and a transform, the
 *   identity at upload.  World vertices = transform . rest.  A transform bitwise equal to the identity uses the rest data
 *   unchanged (no arithmetic: -0.0 stays -0.0).  Otherwise, per row r of the row-major 3x4 m (DXR's Transform[3][4]):
 *   x'_r = ((m[4r]*x + m[4r+1]*y) + m[4r+2]*z) + m[4r+3] in float, no fused multiply-add; normals are multiplied by the inverse
 *   transpose of the 3x3, computed on the host in double and rounded to float once, and are not renormalised.
 * - Updates are staged; one refit covers all of them.  It runs on the context's stream before the next call that reads the tree
 *   or the records: every render entry point, crt_trace_rays* / crt_occluded_rays*, crt_bvh_info* / crt_bvh_export*,
 *   crt_mesh_vertices; crt_refit forces it.  The refit keeps the tree's shape and leaf order and recomputes the leaf-ordered
 *   triangle / shading records (each byte-equal to what a build of the moved meshes writes for that triangle), the binary boxes
 *   bottom-up, the wide tree (whose node count and depth may change) and its plane table.  Like a re-upload it resets
 *   accumulation and the stored launch orders.  A scene that moves far from where it was built traces slower than a rebuilt one.
 * - Errors: NULL ctx -> CRT_EINVAL; no scene, or a scene uploaded without "dynamic" -> CRT_ESTATE; CRT_EINVAL for a bad mesh
 *   index, n_vertices other than the uploaded count, xyz == NULL, normals for a mesh uploaded without normals, a non-finite
 *   matrix entry, a singular 3x3 on a mesh that has normals.  A failed call changes nothing.
 * - Several ranks (crt_comm_*): each rank's context applies the updates it is given; nothing is propagated between ranks. */
int crt_update_vertices(crt_ctx* ctx, uint32_t mesh, uint32_t n_vertices, const float* xyz, const float* normals /* NULL = keep */);
/* the same from device memory: the caller makes d_xyz / d_normals ready on the context's stream; they are read during the call */
int crt_update_vertices_device(crt_ctx* ctx, uint32_t mesh, uint32_t n_vertices, const void* d_xyz, const void* d_normals);
int crt_set_mesh_transform(crt_ctx* ctx, uint32_t mesh, const float m[12]); /* row-major 3x4; NULL = identity */
int crt_refit(crt_ctx* ctx, double* device_ms /* may be NULL: HIP-event time of the refit, 0 when nothing was pending */);
/* Rebuild (DXR: BuildRaytracingAccelerationStructure without PERFORM_UPDATE): applies the pending updates, then builds a new tree
 * on the GPU from the world vertices already in HBM, with the builder option "gpu_builder" names (0 = LBVH, the default; 1 = PLOC).
 * Nothing is read back from the caller.
 * - The tree and every record equal, byte for byte, what a "gpu_build" = 1 upload of the moved meshes with the same builder
 *   produces; uv records follow their triangles.  Later refits refit the new tree.
 * - Like a refit it gives the scene a new serial (accumulation and the stored launch orders restart) and updates the root box,
 *   crt_bvh_info / crt_bvh_info4.  Synchronous; it works whether or not anything was pending.
 * - Pick it over crt_refit when the meshes moved far from where the tree was built (a refitted tree keeps its shape and traces
 *   slower the further the geometry moves); a refit is cheaper when the motion is small.
 * - Errors: NULL ctx -> CRT_EINVAL; no scene, or a scene uploaded without "dynamic" -> CRT_ESTATE; HIP failures -> CRT_EHIP, after
 *   which the context has no scene (as after a failed upload). */
int crt_rebuild(crt_ctx* ctx, double* device_ms /* may be NULL: HIP-event time from the first transform to the collapsed tree */);
/* world-space vertices (and normals, may be NULL) of a mesh as they are traced, n_vertices * 3 floats each */
int crt_mesh_vertices(const crt_ctx* ctx, uint32_t mesh, float* xyz, float* normals);

/* ---- motion: where a pixel's surface element was in the previous frame, for scenes whose meshes move (DXR renderers compute
 * motion vectors from the previous frame's instance transforms; here the previous world vertices themselves are kept, so
 * crt_update_vertices deformations are covered too).  Dynamic scenes only (option "dynamic").  The per-frame loop:
 *     1. render frame f;                       2. crt_motion_snapshot;
 *     3. move the meshes (crt_update_vertices*, crt_set_mesh_transform);
 *     4. render frame f + 1 and its guides;    5. crt_frame_motion (or crt_previous_points on ids the caller already has);
 *     6. crt_temporal_accumulate_motion with those points.
 * - crt_motion_snapshot applies pending refits, as the queries do, then copies the current world vertices of every mesh (12 B
 *   per vertex) into a context-owned "previous" buffer, on the context's stream.  The buffer is allocated by the first call and
 *   freed by the next upload or by crt_destroy; between an upload and the first snapshot there is none and every triangle counts
 *   as "not moved".  It is indexed by vertex (topology and vertex numbering are fixed at upload), so it survives crt_refit and
 *   crt_rebuild with either builder; crt_update_vertices* and crt_set_mesh_transform never touch it.  NULL ctx -> CRT_EINVAL; no
 *   scene, or a scene uploaded without "dynamic" -> CRT_ESTATE.  A context that never calls it allocates nothing and behaves as
 *   without it.
 * - crt_previous_points*: n records of inst / prim (uint32) and uv (2 floats), exactly as crt_trace_rays*, crt_shade_rays* and
 *   crt_list_hits* write them; point: 3 floats per record.  Let i0, i1, i2 be the triangle's mesh-local indices, q0, q1, q2 its
 *   world vertices at the last snapshot and c0, c1, c2 its current ones (after pending refits).  The output is three quiet NaNs
 *   (bits 0x7FC00000), "not moved / unknown", when inst == CRT_MISS, inst >= the number of meshes, prim >= that mesh's triangle
 *   count, u or v is NaN, no snapshot exists, the nine floats of q equal the nine of c bitwise, or any component of the result is
 *   not finite (an inert triangle).  Otherwise, per component,
 *       point = fmaf(v, q2 - q0, fmaf(u, q1 - q0, q0))
 *   with each difference rounded once and no other fused multiply-add: the form crt_closest_points uses for its point.
 *   tests/motion_reference.c restates it in C; the kernel equals it bit for bit.
 *   The results depend on the vertex buffers and the indices alone -- not on the tree, the builder, refit versus rebuild or the
 *   order of the records.  n = 0 returns CRT_OK and launches nothing.  CRT_ESTATE without a dynamic scene.  CRT_EINVAL for a NULL
 *   ctx or buffer or a misaligned device pointer (uv 8-byte, the rest 4-byte); these checks come before the refit.
 *   stats (may be NULL): kernel_ms, total_ms, rays_primary = n; every other count is zero.
 * - crt_frame_motion*: width * height * 3 floats, row-major: bit for bit crt_previous_points applied to the inst / prim / uv that
 *   crt_trace_rays reports for the CRT_SAMPLE_CENTRE records of crt_camera_rays -- the ray whose t crt_frame_guides reports.  The
 *   camera-ray kernel, the closest-hit query and the previous-points kernel run back to back; temporary memory: 48 B per pixel
 *   (records, uv, inst, prim) in the context's query arena of the stream.  CRT_EINVAL as for crt_frame_guides (width or height
 *   0, width * height > 2^28, a NULL buffer, a device pointer that is not 4-byte aligned), CRT_ESTATE without a dynamic scene;
 *   these checks come before the refit.  Camera, mode, accumulation sums, launch orders and frame outputs are untouched.
 *   stats: kernel_ms = the three kernels together, rays_primary = width * height; with crt_set_counting(ctx, 1) nodes_visited /
 *   tris_tested as crt_trace_rays counts them.
 *   The cheaper route: a caller who already has inst / prim / uv of the camera rays (crt_shade_rays on the crt_camera_rays
 *   records gives guides and ids in one launch) calls crt_previous_points and pays no second trace.
 * - crt_temporal_accumulate_motion*: crt_temporal_accumulate* with prev_point (3 floats per pixel, 4-byte aligned device
 *   pointer; may be NULL).  With NULL, and with a buffer of NaNs, the result equals crt_temporal_accumulate* bit for bit.  The
 *   contract is the twelve steps above with these changes:
 *    4'. m = prev_point[p];  moved = all three components of m are finite;  P as in step 4;  Pm = moved ? m : P.
 *    5'. v = Pm - o_prev.
 *    7'. The static-camera shortcut (fx = px, fy = py, steps 5 and 6 skipped) applies to a pixel only when the cameras are equal
 *        bitwise and the pixel is not moved.  A moved pixel always projects.
 *    9'. The plane test is |dot(n_p, Pq - Pm)| <= depth_tolerance * t_p.  The normal test is unchanged.
 *   Liveness, demodulation, taps, sums, blend and the history record stay as they are.
 * - The remaining limit: history normals are the previous frame's, so a surface that rotates by more than
 *   acos(normal_threshold) per frame drops its history (conservative).  Between two frames a surface either moved rigidly or did
 *   not move; the plane test with n_p is exact for translations and approximate for rotations.  Previous normals and
 *   rotation-aware tests are out of scope.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variants: synchronous, staged. */
int crt_motion_snapshot(crt_ctx* ctx);
int crt_previous_points_device(crt_ctx* ctx, uint32_t n, const void* d_inst, const void* d_prim, const void* d_uv, void* d_point,
                               crt_frame_stats* stats);
int crt_previous_points(crt_ctx* ctx, uint32_t n, const uint32_t* inst, const uint32_t* prim, const float* uv, float* point,
                        crt_frame_stats* stats);
int crt_frame_motion_device(crt_ctx* ctx, uint32_t width, uint32_t height, void* d_prev_point, crt_frame_stats* stats);
int crt_frame_motion(crt_ctx* ctx, uint32_t width, uint32_t height, float* prev_point, crt_frame_stats* stats);
int crt_temporal_accumulate_motion_device(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12],
                                          const float cam_prev[12], const void* d_rgb, const void* d_normal, const void* d_albedo,
                                          const void* d_t, const void* d_prev_point /* NULL = nothing moved */,
                                          const void* d_hist_prev /* NULL = no history */, void* d_hist_next,
                                          void* d_out /* may be NULL */, const crt_temporal_params* params /* NULL = defaults */,
                                          crt_frame_stats* stats);
int crt_temporal_accumulate_motion(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12], const float cam_prev[12],
                                   const float* rgb, const float* normal, const float* albedo, const float* t, const float* prev_point,
                                   const float* hist_prev, float* hist_next, float* out, const crt_temporal_params* params,
                                   crt_frame_stats* stats);

/* ---- gradients: the backward pass of crt_trace_rays* and crt_closest_points* (no reference counterpart; what a differentiable
 * renderer's ray cast gives a fitting loop).  A caller moves the vertices (crt_update_vertices*), queries, forms a loss on t / uv
 * or on dist and gets dL/d(record) and dL/d(vertex) back: fitting a mesh to depth or lidar returns, pose estimation, training
 * against a distance field.  Dynamic scenes only (option "dynamic"): the world vertices by vertex, the mesh-local indices and the
 * mesh table are what such a scene keeps in HBM.
 * - Inputs, n records each: the ray or point records of the forward call, and inst / prim / t / uv (points: inst / prim / uv)
 *   exactly as the forward call wrote them -- or edited: nothing is traced again, a record names its triangle by (inst, prim).
 *   grad_t (n floats) and grad_uv (n x 2 floats) are dL/dt and dL/d(u, v); either may be NULL (= zeros), not both.  grad_dist
 *   (n floats) is dL/ddist.
 * - Ray hit.  The hit satisfies o + t d = a + u (b - a) + v (c - a) with a, b, c the triangle's current world vertices (after
 *   pending refits), d not normalised and t parametric, as crt_trace_rays defines them.  With e1 = b - a, e2 = c - a,
 *   n = e1 x e2, w = 1 - u - v and g = (g_t, g_u, g_v), implicit differentiation gives
 *       det = -(d . n),   lambda = (g_t n + g_u (d x e2) + g_v (e1 x d)) / det,
 *       dL/do = lambda,  dL/dd = t lambda,  dL/da = -w lambda,  dL/db = -u lambda,  dL/dc = -v lambda.
 *   grad_rays: 8 floats per record {dL/do, 0, dL/dd, 0}, the layout of the ray record (tmin and tmax get no gradient).
 * - Closest point.  dist = |p - q| with q = w a + u b + v c the minimiser over the triangle; by the envelope theorem, with
 *   nhat = (p - q) / dist and s = g nhat:  dL/dp = s,  dL/da = -w s,  dL/db = -u s,  dL/dc = -v s.  Only dist is differentiable
 *   this way; point, uv, inst and prim have no gradient.  grad_points: 4 floats per record {dL/dp, 0} (rmax gets none).
 * - Operation order (float32, no fused multiply-add except where fmaf is written, / and sqrtf correctly rounded), per record:
 *     e1_k = b_k - a_k, e2_k = c_k - a_k, each rounded once;
 *     a cross product x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0): two products and one subtraction per component;
 *     n = e1 x e2, P = d x e2, Q = e1 x d;  det = -((d0 n0 + d1 n1) + d2 n2);
 *     num_k = (g_t n_k + g_u P_k) + g_v Q_k;  lambda_k = num_k / det;  dL/dd_k = t lambda_k;
 *     w = (1 - u) - v;  the vertex contributions are -(w lambda_k), -(u lambda_k), -(v lambda_k).
 *   Points:  q_k = fmaf(v, c_k - a_k, fmaf(u, b_k - a_k, a_k)), the form crt_closest_points uses for its point;  r_k = p_k - q_k;
 *     len = sqrtf((r0 r0 + r1 r1) + r2 r2);  nhat_k = r_k / len;  s_k = g nhat_k;  contributions -(w s_k), -(u s_k), -(v s_k).
 *   tests/grad_reference.c restates this in C; grad_rays and grad_points equal it bit for bit.
 * - A record is inert -- its grad_rays / grad_points entry is all +0.0 and it adds nothing to any vertex -- when
 *   inst == CRT_MISS or inst >= the number of meshes; prim >= that mesh's triangle count; any of t, u, v, g_t, g_u, g_v (points: u,
 *   v, g), lambda_k, t lambda_k (points: s_k) is not finite; or, for points, len is 0 or not finite.  A miss of crt_trace_rays
 *   with tmax = +inf is inert by its t; a ray parallel to its triangle's plane (det = 0) by its lambda; a triangle with a
 *   non-finite vertex by its lambda.  len is computed here from p, u, v and the current vertices, not read from the forward call's
 *   dist: a point that lies on the surface only up to rounding has a tiny len and gets a unit vector of rounding noise times g --
 *   the derivative of a distance has no direction at zero.
 * - grad_xyz: 3 floats per vertex, all meshes back to back in upload order -- the order of the concatenated crt_mesh_vertices
 *   results; mesh m starts at the sum of the vertex counts of the meshes before it.  It is the gradient with respect to the WORLD
 *   vertices (a caller who moves rest vertices under a transform multiplies by the transposed 3x3).  It is overwritten, not
 *   accumulated: a vertex no live record touches reads exactly +0.0.
 *   Each float32 contribution is widened to float64 and added with the hardware float64 atomic add to a context-owned array of 3
 *   doubles per vertex (allocated by the first call that asks for grad_xyz, freed by the next upload or by crt_destroy, zeroed per
 *   call; a context that never asks allocates nothing); a second kernel rounds each sum to float32 once.  The result is the
 *   correctly rounded float32 of the exact sum of the contributions unless that sum lies within m * 2^-52 * sum|c_i| of a
 *   rounding boundary, for m contributions: independent of the order of the records and of scheduling up to that rare last bit,
 *   not promised bit-reproducible.  Calls of one context share the array: a call waits (on the GPU) for the one before it.
 * - Nothing depends on the tree, the builder or refit versus rebuild: only the vertex buffer and the indices are read.
 * - Scene scale: with vertices, origins, t, points times 2^k and a fixed loss -- g_t and grad_dist times 2^-k, g_u and g_v as they
 *   are -- the formulas above give dL/do, dL/dp and the vertex contributions times 2^-k and dL/dd unchanged, bit for bit while
 *   every intermediate stays a normal float (n and det are quadratic in a length).  Measured with the forward query's outputs
 *   at that scale as inputs (tests/test_scale_similarity.py): the forward query's own range, k = -34 .. 41
 *   for rays and -28 .. 30 for points.  Outside it kernel and reference still agree bit for bit.
 * - Pending refits are applied first.  n = 0 returns CRT_OK and launches nothing (no buffer is looked at, grad_xyz is not
 *   written); n up to 2^32 - 1.  CRT_ESTATE without a dynamic scene.  CRT_EINVAL for a NULL ctx, a NULL input buffer, grad_t and
 *   grad_uv both NULL, grad_rays (grad_points) and grad_xyz both NULL, or a misaligned device pointer: rays, points, grad_rays and
 *   grad_points 16-byte, uv and grad_uv 8-byte, the rest 4-byte.  These checks come before the refit.
 * - stats (may be NULL): kernel_ms (the zeroing, the record kernel and the rounding kernel), total_ms, rays_primary = n; every
 *   other count is zero.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variants: synchronous, staged. */
int crt_trace_rays_backward_device(crt_ctx* ctx, uint32_t n, const void* d_rays, const void* d_inst, const void* d_prim,
                                   const void* d_t, const void* d_uv, const void* d_grad_t /* may be NULL = zeros */,
                                   const void* d_grad_uv /* may be NULL = zeros */, void* d_grad_rays /* may be NULL */,
                                   void* d_grad_xyz /* may be NULL */, crt_frame_stats* stats);
int crt_trace_rays_backward(crt_ctx* ctx, uint32_t n, const float* rays, const uint32_t* inst, const uint32_t* prim, const float* t,
                            const float* uv, const float* grad_t, const float* grad_uv, float* grad_rays, float* grad_xyz,
                            crt_frame_stats* stats);
int crt_closest_points_backward_device(crt_ctx* ctx, uint32_t n, const void* d_points, const void* d_inst, const void* d_prim,
                                       const void* d_uv, const void* d_grad_dist, void* d_grad_points /* may be NULL */,
                                       void* d_grad_xyz /* may be NULL */, crt_frame_stats* stats);
int crt_closest_points_backward(crt_ctx* ctx, uint32_t n, const float* points, const uint32_t* inst, const uint32_t* prim,
                                const float* uv, const float* grad_dist, float* grad_points, float* grad_xyz, crt_frame_stats* stats);

/* ---- variance: luminance moments carried with the history, a per-pixel variance from them, and the a-trous filter with a colour
 * weight that follows that variance (Schied et al. 2017, "Spatiotemporal Variance-Guided Filtering").  The filter's weight is wide
 * where the estimate is noisy (short history, disocclusion, frame edges) and closes where the history has converged.
 * - crt_temporal_variance*: crt_temporal_accumulate_motion* plus three buffers.  mom_prev / mom_next: 2 floats {m1, m2} per
 *   pixel (8-byte aligned on the device), the running mean of the luminance and of its square; the caller owns two such buffers
 *   and swaps them with the history buffers.  mom_prev is NULL exactly when hist_prev is.  variance: 1 float per pixel (4-byte
 *   aligned).  prev_point may be NULL.  The context keeps no state.  The contract is the twelve steps of crt_temporal_accumulate,
 *   with 4', 5', 7' and 9' when prev_point is given, and these; the arithmetic rules are the same:
 *    V1. For a live pixel, with c of step 2:  l = fmaf(0.0722, c.b, fmaf(0.7152, c.g, 0.2126 * c.r));  q = l * l.
 *    V2. A pixel that is not live: mom_next = {0, 0}, variance = 0.
 *    V3. Step 9 gains a condition: a tap is valid only if m1 and m2 of its mom_prev record are finite.  When every moment
 *        record is finite, hist_next and out equal crt_temporal_accumulate_motion* on the same inputs bit for bit.
 *    V4. Step 10 gains SM1 = sum b_k * m1_q and SM2 = sum b_k * m2_q (a product, then a sum), over the same valid taps in the
 *        same order, each starting at 0.
 *    V5. With history (step 11's condition): a_m = max(alpha_moments, 1 / (L + 1));  h1 = SM1 / W, h2 = SM2 / W;
 *        m1 = fmaf(a_m, l - h1, h1), m2 = fmaf(a_m, q - h2, h2).  Without: m1 = l, m2 = q.  mom_next = {m1, m2}.
 *    V6. The variance, a second pass over the records V1 to V5 and step 12 wrote.  For a live pixel p with len = hist_next[p].len:
 *        len >= min_history:  variance = fmaxf(m2 - m1 * m1, 0) (a product, then a difference).
 *        Otherwise a spatial estimate over the 7 x 7 window around p, dy = -3..3 outer, dx = -3..3 inner, the centre included.
 *        The centre always counts.  Another tap q counts when it is inside the image, hist_next[q].len > 0, the 8 floats of
 *        hist_next[q] and the 2 of mom_next[q] are finite, |dot(n_p, Pq - P)| <= depth_tolerance * t_p with Pq = o_cur +
 *        dir(rot_cur, qx, qy) * t_q and P of step 4, and dot(n_p, n_q) >= normal_threshold.  N = the number of counted taps as
 *        a float, A1 = sum m1_q, A2 = sum m2_q in tap order from 0, M1 = A1 / N, M2 = A2 / N.
 *        variance = fmaxf(M2 - M1 * M1, 0) * ((float)min_history / len).
 *        The value is written as computed: a luminance that overflowed shows.
 *   tests/variance_reference.c restates all of it in C; the kernels equal it bit for bit.
 *   Aliasing: d_out may equal d_rgb; d_hist_next must not overlap d_hist_prev nor d_mom_next d_mom_prev; no other two buffers
 *   may overlap.  CRT_EINVAL as for crt_temporal_accumulate_motion*, and for alpha_moments outside [0, 1] or NaN; min_history
 *   outside 1..2^24; a NULL mom_next or variance; exactly one of hist_prev and mom_prev NULL; a misaligned device pointer
 *   (history: 16-byte, moments: 8-byte, the rest: 4-byte).  A failed call launches nothing and writes nothing.
 *   Two kernels, no scratch memory, no atomics: the same input gives the same bits.
 * - crt_denoise_variance*: crt_denoise* with variance (1 float per pixel) as a further input and variance_out (1 float per
 *   pixel; may be NULL) as a further output.  The variance is that of the luminance of the colour that is filtered: demodulate
 *   must be what the crt_temporal_variance call that made it was given.
 *     Live: crt_denoise's rule, and variance finite and >= 0.  A pixel that is not live is copied rgb -> out and variance ->
 *       variance_out bit for bit and is never a tap.
 *     Start: a and c_0 as in crt_denoise;  v_0 = variance;  lum(c) as l in V1.
 *     Pass i = 0 .. iterations - 1, stride s = 2^i, for a live centre p:
 *       g_p = the 3 x 3 mean of v_i at stride 1 whatever s, weights (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), over the taps inside the
 *             image and live, divided by the sum of the weights used
 *       d_p = sigma_luminance * sqrt(g_p) + 1e-4
 *       for the 25 taps of crt_denoise (inside the image and live):
 *         e = |lum(c_i(p)) - lum(c_i(q))| / d_p + |n_p - n_q|^2 / sigma_normal^2 + ((t_p - t_q) / (sigma_depth t_p))^2
 *         w = h[dx + 2] h[dy + 2] exp(-e)
 *       c_{i+1}(p) = sum w c_i(q) / sum w        v_{i+1}(p) = sum w^2 v_i(q) / (sum w)^2
 *       sigma_luminance is not halved: the variance shrinks by itself every pass.
 *     Output: out = c_N a;  variance_out = v_N.
 *   Float32 throughout; no bit-for-bit contract against a CPU form (exp).  What holds: crt_denoise's deviation bound against a
 *   float64 evaluation, for out and variance_out (tests/test_variance.py); determinism; host form = device form = in-place form
 *   bit for bit.  Aliasing: d_out may equal d_rgb, d_variance_out may equal d_variance; no other two buffers may overlap.
 *   CRT_EINVAL as for crt_denoise (sigma_luminance in sigma_color's place: > 0, +inf switches the term off) and for a NULL
 *   variance.  Scratch as for crt_denoise: 48 B per pixel, the guide plane {n, t} and two colour planes {c, v}.
 * Both: params == NULL means the defaults; stats (may be NULL): kernel_ms, total_ms, every count zero; no scene is needed; the
 * context's camera, mode, accumulation sums, launch orders and frame outputs are untouched.
 * *_device: asynchronous on the context's stream unless stats != NULL.  Host variants: synchronous, staged. */
typedef struct crt_temporal_variance_params {
    crt_temporal_params base;
    float alpha_moments;   /* default 0.2: least weight of the new frame's luminance moments */
    uint32_t min_history;  /* default 4, 1..2^24: below this history length the variance is the spatial estimate */
} crt_temporal_variance_params;
typedef struct crt_denoise_variance_params {
    uint32_t iterations;    /* 1..8, default 5: pass i samples at stride 2^i */
    float sigma_luminance;  /* default 0.0625: luminance differences are measured in this many standard deviations */
    float sigma_normal;     /* default 0.3 */
    float sigma_depth;      /* default 0.05, relative to the centre pixel's t */
    uint32_t demodulate;    /* default 1; must match the crt_temporal_variance call's */
} crt_denoise_variance_params;
int crt_temporal_variance_device(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12], const float cam_prev[12],
                                 const void* d_rgb, const void* d_normal, const void* d_albedo, const void* d_t,
                                 const void* d_prev_point /* NULL = nothing moved */, const void* d_hist_prev /* NULL = no history */,
                                 void* d_hist_next, const void* d_mom_prev /* NULL with d_hist_prev */, void* d_mom_next,
                                 void* d_variance, void* d_out /* may be NULL */,
                                 const crt_temporal_variance_params* params /* NULL = defaults */, crt_frame_stats* stats);
int crt_temporal_variance(crt_ctx* ctx, uint32_t width, uint32_t height, const float cam_cur[12], const float cam_prev[12],
                          const float* rgb, const float* normal, const float* albedo, const float* t, const float* prev_point,
                          const float* hist_prev, float* hist_next, const float* mom_prev, float* mom_next, float* variance,
                          float* out, const crt_temporal_variance_params* params, crt_frame_stats* stats);
int crt_denoise_variance_device(crt_ctx* ctx, uint32_t width, uint32_t height, const void* d_rgb, const void* d_normal,
                                const void* d_albedo, const void* d_t, const void* d_variance, void* d_out,
                                void* d_variance_out /* may be NULL */, const crt_denoise_variance_params* params /* NULL = defaults */,
                                crt_frame_stats* stats);
int crt_denoise_variance(crt_ctx* ctx, uint32_t width, uint32_t height, const float* rgb, const float* normal, const float* albedo,
                         const float* t, const float* variance, float* out, float* variance_out,
                         const crt_denoise_variance_params* params, crt_frame_stats* stats);

/* ---------------------------------------------------------------------------------------------------
 * Scene layer: stands in for CRTScene / CRTSceneParser / CRTCamera (kept API surface, host only, no GPU)
 * ------------------------------------------------------------------------------------------------- */
typedef struct crt_scene crt_scene;

/* CRTScene::CRTScene(file) -> CRTSceneParser::parseScene (R/CRTScene.cpp:7-15, R/CRTSceneParser.cpp:407-427).
 * Accepts .crtscene (JSON) and, as extensions, .obj and the binary cache .crtbin. Absent optional keys take defaults instead of the
 * reference's undefined behaviour. */
int crt_scene_load(const char* path, crt_scene** out, char* err, size_t err_len);
/* binary scene cache (.crtbin): writes everything a .crtscene yields, vertex normals included,
 * as raw arrays; crt_scene_load reads it back by extension at memcpy speed */
int crt_scene_save(const crt_scene* s, const char* path, char* err, size_t err_len);
/* empty scene to be filled programmatically */
int crt_scene_new(crt_scene** out);
void crt_scene_free(crt_scene* s);
/* CRTMesh::addVertex/addIndex/setMaterialIndex + calculateVertexNormals (R/CRTMesh.cpp:6-24,66-94) */
int crt_scene_add_mesh(crt_scene* s, const float* xyz, uint32_t n_vertices, const uint32_t* idx, uint32_t n_triangles,
                       int32_t material_index);
int crt_scene_add_light(crt_scene* s, const float pos[3], float intensity);
int crt_scene_add_material(crt_scene* s, const crt_material* m);

uint32_t crt_scene_mesh_count(const crt_scene* s);                               /* getObjects().size() */
int crt_scene_mesh(const crt_scene* s, uint32_t i, crt_mesh_view* out);          /* views into scene-owned memory */
uint32_t crt_scene_light_count(const crt_scene* s);                              /* getLights() */
int crt_scene_light(const crt_scene* s, uint32_t i, crt_light* out);
uint32_t crt_scene_material_count(const crt_scene* s);                           /* getMaterials() */
int crt_scene_material(const crt_scene* s, uint32_t i, crt_material* out);
uint32_t crt_scene_texture_count(const crt_scene* s);                            /* getTextures().size() */
/* CRTTexture::getColor(u, v) of texture i (R/CRTTexture*.cpp), evaluated on the host */
int crt_scene_texture_color(const crt_scene* s, uint32_t i, float u, float v, float out_rgb[3]);
/* programmatic textures: type = "albedo" | "edges" | "checker" | "bitmap" (file_path: binary PPM); a material refers to one by name */
int crt_scene_add_texture(crt_scene* s, const char* name, const char* type, const float color_a[3], const float color_b[3], float scalar,
                          const char* file_path);
int crt_scene_set_material_texture(crt_scene* s, uint32_t material, const char* texture_name);
int crt_scene_set_mesh_uvs(crt_scene* s, uint32_t mesh, const float* uvs /* n_vertices * 3 */);
int crt_scene_settings(const crt_scene* s, uint32_t* width, uint32_t* height, float background_rgb[3]); /* getSettings() */

/* CRTCamera (R/CRTCamera.h:5-32, .cpp:9-130) on the scene's camera */
int crt_scene_camera_get(const crt_scene* s, float pos[3], float rot[9]);
int crt_scene_camera_set(crt_scene* s, const float pos[3], const float rot[9]);
int crt_scene_camera_rotate(crt_scene* s, float delta_yaw_deg, float delta_pitch_deg);
int crt_scene_camera_zoom(crt_scene* s, float amount);
int crt_scene_camera_move_forward(crt_scene* s, float distance);
int crt_scene_camera_move_right(crt_scene* s, float distance);
int crt_scene_camera_pan(crt_scene* s, float degrees);
int crt_scene_camera_tilt(crt_scene* s, float degrees);
int crt_scene_camera_roll(crt_scene* s, float degrees);
int crt_scene_camera_pan_around_target(crt_scene* s, float degrees, const float target[3]);

/* convenience: crt_upload_scene + crt_set_camera from a loaded scene (what DXRTRenderer::createScene +
 * create*Buffers + createAccelerationStructures do with the CRTScene it owns, R/DXRTRenderer.cpp:243-246) */
int crt_upload_scene_from(crt_ctx* ctx, const crt_scene* s);
int crt_set_camera_from(crt_ctx* ctx, const crt_scene* s);

#ifdef __cplusplus
}
#endif
#endif
