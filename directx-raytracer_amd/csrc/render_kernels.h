// Launch interface between the C-ABI layer (crt_api.cpp and the api_*.cpp units, host C++: crt_ctx.h maps them) and the HIP kernels (render_kernels.hip, path_kernels.hip; device code shared through traversal.hip.h / shading.hip.h).
// The frame kernels and the image-space kernels have one launch function each; the persistent query kernels share one
// (launchQuery, query_launch.cpp) over a table of their host stubs (QueryKind, QueryKernel): a kernel file states its rows.
#pragma once

#include <cstddef>
#include <cstdint>

struct ihipStream_t;

namespace crt {

constexpr int kMaxBatch = 4;       // frames per launch (crt_render_tiles_batch_device)
constexpr int kTile = 16;          // macro tile edge: one 256-thread workgroup = 4 wavefronts of 8x8 pixels
constexpr int kStackEntries = 32;  // largest LDS part of the per-lane stack (option "stack_entries"); a lane can hold 3 * depth4 + 1 entries, the rest spills
// Decoded plane table: row i = float(q) of the 24 plane bytes of node i (bytes 24..47 of its record, in
// order: qlo_x qhi_x qlo_y qhi_y qlo_z qhi_z, child k in byte k of each word), 8 floats of zero padding: 128 bytes per
// node, so that a row is one s_load_dwordx16 + one s_load_dwordx8 on 64-byte boundaries.  Read by scalar-path node steps only.
constexpr uint32_t kPlaneStride = 32;

struct RenderParams {
    // scene (HBM)
    const void* nodes;   // crt_bvh_node4q[n_nodes], 64 B (the quantised wide tree)
    const void* tris;    // crt_bvh_tri[n_tris], 48 B
    const float* planes; // the decoded plane table, kPlaneStride floats per node (launchDecodePlanes)
    const void* shade;   // crt_bvh_shade[n_tris], 48 B
    const void* lights;  // crt_light[n_lights]
    const void* mats;    // crt_material[n_mats] (28 B)
    const void* uvs;     // crt_bvh_uv[n_tris] (24 B, leaf order) or null
    const void* textures; // TextureRec[n_textures] (below), bitmaps' texels in `texels`
    const unsigned char* texels;
    uint32_t n_textures;
    uint32_t n_nodes, n_tris, n_lights, n_mats;
    // per-frame constants: CameraCB (R/DXRTRenderer.h:54-59) + DebugCB (:68-72)
    float pos[3];
    float rot[9];
    float miss[3];
    uint32_t mode;
    uint32_t spp, max_bounces, seed; // mode 200 (path tracing)
    float phong_ks;                  // mode 100: specular coefficient (0 = plain Lambert), options "phong_ks" / "phong_exponent"
    uint32_t phong_exp;
    uint32_t width, height;
    // tiling
    uint32_t tiles_x, tiles_y;   // ceil(width/16), ceil(height/16)
    uint32_t rank, n_ranks;      // this launch renders macro tiles k with k % n_ranks == rank
    uint32_t n_local_tiles;      // grid size: number of such tiles
    uint32_t staging;            // 0: write row-major frame buffers; 1: rgba8 goes to the tile-major staging buffer
    uint32_t tune_inner_min;     // wave scheduling knob of the closest-hit traversal, see closestIteration() (int: negative = adaptive)
    uint32_t tune_inner_min_any; // the same for the any-hit (shadow ray) traversal
    uint32_t stack_entries;      // per-lane stack entries kept in LDS; deeper ones go to the spill arena
    uint32_t wide_offsets;       // wideOffsets() below: 1 = the render kernel's per-lane fetches keep 64-bit address arithmetic
    uint32_t debug_skip_units;   // diagnostics: with unit_order, the first N work units are not rendered
    uint32_t boost_units;        // with unit_order: the first boost_units (most expensive) work units run at raised priority
    uint32_t split_units;        // with unit_order: the first split_units work units are rendered by FOUR wavefronts, one per 4x4
                                 // quarter of the 8x8 packet, every ray by four lanes (four segments of its way through the scene)
    uint32_t split_rays_log2;    // rays (pixels) per wavefront of a split packet: 4 -> 16 (four wavefronts per packet), 3 -> 8, 2 -> 4 (sixteen)
    uint32_t split_segs_log2;    // pieces a split ray is cut into: 2 -> 4, 3 -> 8, 4 -> 16
    float scene_lo[3], scene_hi[3]; // the scene's box (root of the tree): where a split ray's segments are cut
    uint32_t xcd_group;          // consecutive tiles of the list handed to one XCD before moving to the next (1..16, power of 2)
    // outputs (device pointers, nullable except rgba8)
    uint32_t* rgba8;
    uint32_t* hit_inst;
    uint32_t* hit_prim;
    float* hit_t;
    float* rgb_f32;
    unsigned long long* counters; // [0] nodes fetched, [1] triangles fetched, [2] shadow rays, [3] closest-hit rays; counting variant
    int* spill;                   // stack spill arena: renderUnitCount() x 64 lanes x spill_stride ints, rarely touched
    uint32_t spill_stride;        // >= 3 * wide depth + 1 - stack_entries: the deepest stack any ray can build
    const uint32_t* unit_order;   // nullable: work units sorted by descending cost of the previous frame (launch order)
    uint32_t* unit_cost;          // nullable: per work unit, traversal-loop iterations of its wavefront (this frame)
    // batch: n_batch frames (1..kMaxBatch) in ONE launch, grid = n_batch x units_per_frame; frame 0 uses pos / rot / rgba8
    // above, frame f > 0 its own camera and output below (hit ids / float colour are frame 0's only)
    uint32_t n_batch;
    uint32_t units_per_frame;
    float batch_pos[3][3];
    float batch_rot[3][9];
    uint32_t* batch_rgba8[3];
    // mode 200: per-workgroup scratch of the wavefront-private path pipeline (path_kernels.hip pathKernel)
    unsigned char* path_scratch;  // pathGridSize() regions of path_region_bytes: one per RESIDENT workgroup of the persistent kernel
    uint32_t* path_counter;       // work-item counter of the launch (zeroed on the stream before it)
    uint32_t path_work_items;     // pathWorkgroupCount(): pixel tiles x frames of the batch
    uint32_t path_ranges;         // 1 or 8: contiguous ranges of the work items, one counter (64 bytes apart) and one home XCD each
    size_t path_region_bytes;     // pathRegionBytes(path_samples)
    uint32_t path_tile;           // 16: one workgroup per 16x16 macro tile; 8: one per 8x8 packet
    uint32_t path_samples;        // samples of the tile carried through the pipeline together: B = tile^2 x this paths (<= 1024)
    // mode 200, wavefront pipeline (path_pipeline 1): the stages as separate launches over global queues (path_kernels.hip)
    uint32_t path_wavefront;      // 1: launchPath runs the wavefront pipeline
    void* wf_shade_q;             // float4 arrays.  3 planes x wf_paths: {o, rng} {d, id | bounce << 25} {t, u, v, tri}
    void* wf_trace_q;         // 2 planes x wf_paths
    void* wf_done;            // wf_paths: a path's radiance so far
    void* wf_thr;             // wf_paths: its throughput
    void* wf_accum;           // nullable: 64 x 2 double2 per work item of a pass, float64 sums of earlier passes (spp > path_samples)
    uint32_t* wf_counts;          // kWfHeadBytes: work counters of the camera launch, then {length, cursor} per queue
    uint32_t wf_paths;            // capacity of a pass in paths = plane stride (pathWavefrontPassItems() x 64 x path_samples)
    uint32_t wf_stride, wf_chunk; // the queues' capacity in entries (= plane stride) and the entries a wavefront reserves per atomic (pathWavefrontLayout)
    uint32_t wf_item0, wf_items;  // the work items of this pass
    uint32_t wf_queue;            // queue a shade / trace launch consumes (it fills wf_queue + 1)
    uint32_t wf_s0;               // first sample of this pass
    unsigned long long* timeline; // counting variant only, nullable: per workgroup {start, end} of s_memrealtime (100 MHz) + XCC id
    // mode 200, progressive accumulation (crt_set_accumulation); acc_sum null = off
    void* acc_sum;                // 2 double2 {x, y}, {z, 0} per output index of the RGBA8 store (pixel of a frame, staging index of a tile share): float64 running sums
    uint32_t acc_base;            // global index of the call's first sample = samples already in the sums
    uint32_t acc_total;           // acc_base + spp: what the sums are divided by
};

// The form of the render kernel's per-lane node and triangle fetches.  The narrow form computes a record's byte offset in 32
// bits, which holds while every record starts below 2^32: 64 * n_nodes <= 2^32 and 48 * n_tris <= 2^32 (the shading records
// are 48 bytes too).  The builders admit 2^28 - 1 triangles, so the wide form stays reachable.  option: "wide_offsets", 0 =
// by the sizes, 1 = always wide.
inline bool wideOffsets(uint64_t n_nodes, uint64_t n_tris, uint32_t option)
{
    return option != 0u || 64u * n_nodes > (1ull << 32) || 48u * n_tris > (1ull << 32);
}

// Enqueue the fused rayGen -> traverse -> shade -> store kernel. counting selects the instrumented variant.
int launchRender(const RenderParams& p, bool counting, ihipStream_t* stream);
// number of work units (= workgroups) launchRender uses for p: size of unit_order / unit_cost
uint32_t renderUnitCount(const RenderParams& p);
// mode 200 (path_kernels.hip): the wavefront-private path pipeline; launchRender forwards to launchPath
int launchPath(const RenderParams& p, bool counting, ihipStream_t* stream);
// mode 200 with accumulation at its limit: the stored sums resolved to RGBA8 (and f32 rgb) without tracing
int launchPathAccumResolve(const RenderParams& p, ihipStream_t* stream);
// mode 200 scratch sizing
size_t pathRegionBytes(uint32_t tile, uint32_t samples_per_pass);
uint32_t pathWorkgroupCount(const RenderParams& p);
// wavefront pipeline: bytes in front of the queues (counters), work items one pass may carry for a budget of paths, and the
// arena a pass of `items` work items needs
constexpr size_t kWfHeadBytes = 4096;
uint32_t pathWavefrontPassItems(const RenderParams& p, uint32_t max_paths);
void pathWavefrontLayout(const RenderParams& p, uint32_t items, uint32_t& chunk, uint32_t& stride);
size_t pathWavefrontBytes(const RenderParams& p, uint32_t items);
uint32_t pathGridSize(const RenderParams& p); // workgroups the persistent path kernel starts: min(work items, what the chip holds at once)
// the decoded plane table of n quantised nodes (crt_bvh_node4q) into planes[n * kPlaneStride] (bvh_gpu.hip)
int launchDecodePlanes(const void* nodes4q, uint32_t n, float* planes, ihipStream_t* stream);
// unit_cost -> unit_order (descending)
int launchSortUnits(const uint32_t* cost, uint32_t* order, uint32_t n, bool xcdAffine, ihipStream_t* stream);
// tile-major gathered buffer -> row-major frame
int launchUntile(const uint32_t* gathered, uint32_t* frame, uint32_t width, uint32_t height, uint32_t n_ranks,
                 uint32_t rank_stride, uint32_t first_slot, ihipStream_t* stream);

// What every persistent query kernel (query.hip.h runQuery) is given: the tree, the caller's records, and the launch's share of
// its arena
struct QueryCommon {
    const void* nodes;            // as RenderParams::nodes / tris
    const void* tris;
    uint32_t n_nodes;
    const void* records;          // n records, 16-byte aligned: rays of 32 bytes {ox, oy, oz, tmin, dx, dy, dz, tmax} or points of 16
    uint32_t n;
    uint32_t* cursor;             // chunks handed out behind the grid's own (zeroed on the stream before the launch)
    unsigned long long* counters; // counting variant: [0] nodes fetched, [1] triangles fetched
    int* spill;                   // stack spill arena: grid x 64 lanes x spill_stride ints
    uint32_t spill_stride;
    uint32_t stack_entries;       // per-lane stack entries kept in LDS
    uint32_t inner_min;           // tune_inner_min (closest hit, closest point) or tune_inner_min_any (the others)
    uint32_t chunk;               // records per cursor reservation (queryLayout)
};
// The kinds of query: one persistent kernel each, in a plain and a counting instantiation.  Every kind's parameter struct
// (below) begins with its QueryCommon
enum QueryKind { kQueryClosestHit = 0, kQueryOcclusion = 1, kQueryClosestPoint = 2, kQueryCount = 3, kQueryOccupancy = 4,
                 kQueryListFill = 5 /* the second traversal of crt_list_hits*: a kernel of its own, not an entry point */,
                 kQueryShade = 6, kQueryPath = 7 /* crt_path_rays*: passes of (record, sample) items */, kQueryWinding = 8,
                 kQueryWhitted = 9 /* crt_shade_rays* and the frames in mode 150 */,
                 kQueryAmbient = 10 /* crt_shade_rays* and the frames in mode 120 */, kQueryKinds };
// What the host knows of a kind's kernel: the host stubs of its two instantiations and the ints per stack entry (the
// closest-point stack keeps each entry's box bound beside its reference: 2; every other kind: 1).  Stated by the file that
// defines the kernel and never written again.  (Not const: hipcc would emit a const row into the device code object too.)
struct QueryKernel {
    const void* plain;
    const void* counted;
    uint32_t entryWords;
};
extern QueryKernel kKernelClosestHit, kKernelOcclusion;                 // ray_kernels.hip
extern QueryKernel kKernelClosestPoint, kKernelCount, kKernelOccupancy; // point_kernels.hip
extern QueryKernel kKernelListFill;                                     // list_kernels.hip
extern QueryKernel kKernelShade;                                        // shade_kernels.hip
extern QueryKernel kKernelPath;                                         // path_query_kernels.hip
extern QueryKernel kKernelWinding;                                      // winding_kernels.hip
extern QueryKernel kKernelWhitted;                                      // whitted_kernels.hip
extern QueryKernel kKernelAmbient;                                      // ao_kernels.hip
// The rest is query_launch.cpp.  The kind's row
const QueryKernel& queryKernel(QueryKind kind);
// workgroups of the kind's kernel the current device holds at once with `stack_entries` of LDS stack per lane (0: unknown)
uint32_t queryResident(QueryKind kind, uint32_t stack_entries);
// records per reservation and grid (persistent: at most `resident` workgroups) of a query of n records
void queryLayout(uint32_t n, uint32_t resident, uint32_t& chunk, uint32_t& grid);
// The launch of `grid` workgroups of one wavefront.  params: the kind's parameter struct.  Nothing is launched for no records
// or no grid.  Returns the HIP error code
int launchQuery(QueryKind kind, const void* params, bool counting, uint32_t grid, ihipStream_t* stream);

// batched ray queries (ray_kernels.hip; crt_trace_rays* / crt_occluded_rays*): closest hit or occlusion of n ray records, over
// the 4-wide tree
struct RayQueryParams {
    QueryCommon c;
    float* t;                     // closest hit, each nullable: t, {u, v} (8-byte aligned), mesh ordinal, triangle of the mesh
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
    unsigned char* occluded;      // occlusion: one byte per ray
};
// The outputs of crt_shade_rays* in every mode (ShadeQueryParams, WhittedQueryParams, AmbientQueryParams): each nullable
struct ShadedOutputs {
    float* rgb;                   // 3 floats per ray: the mode's colour, the miss colour on a miss
    float* normal;                // 3 floats per ray: Surface::N, zero on a miss
    float* albedo;                // 3 floats per ray: Surface::albedo, zero on a miss
    float* t;                     // as RayQueryParams'
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
};
// shaded ray queries (shade_kernels.hip; crt_shade_rays*): closest hit of n ray records, then the context's shading mode at
// the hit -- the frames' shading (shading.hip.h) for caller-supplied rays.  Every output is nullable
struct ShadeQueryParams {
    QueryCommon c;                // records: the rays; inner_min: tune_inner_min (the closest-hit phase)
    uint32_t inner_min_any;       // tune_inner_min_any (the shadow-ray phases)
    // the scene's shading tables and the shading state, as RenderParams'
    const void* shade;
    const void* lights;
    const void* mats;
    const void* uvs;
    const void* textures;
    const unsigned char* texels;
    uint32_t n_textures, n_lights, n_mats;
    float miss[3];
    uint32_t mode;                // < 200
    float phong_ks;
    uint32_t phong_exp;
    ShadedOutputs out;
};
// path-traced ray queries (path_query_kernels.hip; crt_path_rays*): one pass of (record, sample) work items, numbered
// sample-major: item = sample-in-pass * n_records + record; c.n = the items of the pass.  Every path leaves its radiance in its
// item's slot of `rad`; launchPathResolve then adds the pass's samples per record in sample order
struct PathQueryParams {
    QueryCommon c;                // records: the rays of the pass's records; inner_min: tune_inner_min (closest-hit phases)
    uint32_t inner_min_any;       // tune_inner_min_any (the shadow-ray phases)
    // the scene's shading tables, as RenderParams'
    const void* shade;
    const void* lights;
    const void* mats;
    const void* uvs;
    const void* textures;
    const unsigned char* texels;
    uint32_t n_textures, n_lights, n_mats;
    float miss[3];
    uint32_t max_bounces, seed;
    const uint32_t* ids;          // path id per record, or NULL: id_base + record
    uint32_t id_base;
    uint32_t n_records;
    uint32_t sample0;             // the sample of the pass's items 0 .. n_records - 1
    void* rad;                    // scratch, one float4 per item: the path's radiance so far, final when it ends
    void* thr;                    // scratch, one float4 per item: its throughput
    float* t;                     // hit outputs as RayQueryParams', written by the items of sample0 (NULL in a call's later passes)
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
};
// Whitted ray queries (whitted_kernels.hip; crt_shade_rays* and the frames in mode 150): the closest hit of n ray records
// followed through mirrors and glass (the specular chain of PathQueryParams' paths, at most max_bounces turns), then mode 100's
// shading at the first surface that is neither.  The outputs are ShadeQueryParams'
struct WhittedQueryParams {
    QueryCommon c;                // records: the rays; inner_min: tune_inner_min (the closest-hit phases)
    uint32_t inner_min_any;       // tune_inner_min_any (the shadow-ray phases)
    // the scene's shading tables, as RenderParams'
    const void* shade;
    const void* lights;
    const void* mats;
    const void* uvs;
    const void* textures;
    const unsigned char* texels;
    uint32_t n_textures, n_lights, n_mats;
    float miss[3];
    uint32_t max_bounces;         // turns a record may take
    float phong_ks;
    uint32_t phong_exp;
    void* state;                  // scratch, kWhittedStateBytes per record: what is touched once per surface -- {T.rgb, k} and
                                  // Phong's view vector
    ShadedOutputs out;
};
constexpr size_t kWhittedStateBytes = 32; // two float4
// a mode-150 or mode-120 frame's RGBA8 from its float colour (3 floats per pixel), the frames' unorm8 rule: n pixels
// (whitted_kernels.hip)
int launchRgbToRgba8(const float* rgb, uint32_t* rgba8, uint32_t n, ihipStream_t* stream);
// Ambient-occlusion ray queries (ao_kernels.hip; crt_shade_rays* and the frames in mode 120): the closest hit of n ray records,
// then `samples` any-hit rays from the hit point over (0, radius) in the first-bounce directions of the mode-200 paths of
// (record, sample, seed); the colour is the share that escapes, or with `sky` mode 100's light plus albedo x miss x that share.
// The outputs are ShadeQueryParams'.  No record state outside the registers
struct AmbientQueryParams {
    QueryCommon c;                // records: the rays; inner_min: tune_inner_min (the closest-hit phase)
    uint32_t inner_min_any;       // tune_inner_min_any (the shadow-ray and occlusion phases)
    // the scene's shading tables, as RenderParams'
    const void* shade;
    const void* lights;
    const void* mats;
    const void* uvs;
    const void* textures;
    const unsigned char* texels;
    uint32_t n_textures, n_lights, n_mats;
    float miss[3];
    float phong_ks;               // sky only: mode 100's specular term
    uint32_t phong_exp;
    uint32_t samples;             // option "ao_samples": 1..4096
    float radius;                 // the occlusion rays' tmax: option "ao_radius" of the root box's diagonal, or 10000
    uint32_t sky;                 // option "ao_sky"
    uint32_t seed;                // option "seed"
    ShadedOutputs out;
};
// The kernels take these structs by value: a member that moves changes their arguments, and with them the device code
static_assert(offsetof(ShadeQueryParams, out) == 176 && sizeof(ShadeQueryParams) == 232, "ShadeQueryParams: layout");
static_assert(offsetof(WhittedQueryParams, out) == 184 && sizeof(WhittedQueryParams) == 240, "WhittedQueryParams: layout");
static_assert(offsetof(AmbientQueryParams, out) == 184 && sizeof(AmbientQueryParams) == 240, "AmbientQueryParams: layout");
static_assert(offsetof(ShadedOutputs, prim) == 48 && sizeof(ShadedOutputs) == 56, "ShadedOutputs: seven pointers");
// rad[sample * n_records + record] of n_samples samples added in sample order to `in` (3 float64 per record; NULL: zero);
// the sums go to `out`, their mean over `total` samples to rgb (each nullable)
int launchPathResolve(const void* rad, uint32_t n_records, uint32_t n_samples, const double* in, double* out, float* rgb, uint32_t total,
                      ihipStream_t* stream);
// point queries (point_kernels.hip; crt_closest_points* / crt_count_hits* / crt_occupancy*): n caller-supplied records, point
// records of 4 floats {x, y, z, rmax} (closest point, occupancy) or ray records (hit counts), over the 4-wide tree
struct PointQueryParams {
    QueryCommon c;
    float* dist;                  // closest point, each nullable: distance, point (3 floats), {u, v} (8-byte aligned), inst, prim
    float* point;
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
    uint32_t* count;              // hit counts: one uint32 per ray
    unsigned char* inside;        // occupancy: one byte per point
    float pad;                    // closest point: absolute pruning margin, 2^-18 x the root box's diagonal
};
// winding numbers (winding_kernels.hip; crt_winding_numbers*): n point records over the 4-wide tree and its moment table,
// kMomentStride floats per node: {p~.xyz, r} of child slots 0..3 (one 64-byte line), then {N~.xyz, 0} of slots 0..3
constexpr uint32_t kMomentStride = 32;
struct WindingQueryParams {
    QueryCommon c;
    const float* moments;         // kMomentStride floats per wide node
    float beta;                   // > 0: a child farther than beta x its radius is taken by its dipole; else every triangle
    float* w;                     // one float per point
};
// the moment table of n_nodes4 quantised nodes, bottom-up over `levels` depth levels (any number >= the wide tree's depth).
// scratch: windingScratchBytes(n_nodes4), the nodes' depths and their float64 sums
size_t windingScratchBytes(uint32_t n_nodes4);
int launchWindingMoments(const void* nodes4q, const void* tris, uint32_t n_nodes4, uint32_t levels, float* moments, void* scratch,
                         ihipStream_t* stream);
// all-hits listing (list_kernels.hip; crt_list_hits*): after the hit counts (kQueryCount), the exclusive
// sum of the counts into 64-bit offsets, a second traversal (kQueryListFill) that writes every accepted hit into its ray's segment, and the
// sort + resolve of every segment.  The three later steps read offsets[n] on the device and leave when it exceeds capacity.
struct ListParams {
    QueryCommon c;                // records: the rays
    const unsigned long long* offsets; // n + 1, written by launchListScan
    unsigned long long capacity;  // records every record array holds
    float* tkey;                  // work arrays of `capacity` records: a hit's prescaled t' and its leaf-order triangle record.
    uint32_t* idkey;              // They may be the caller's t and prim arrays (resolved in place) or scratch.
    float* t;                     // outputs, each nullable
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
    uint32_t* longRays;           // n entries (the count buffer, free once the offsets exist): rays left to the wavefront sort
    uint32_t* longCount;          // their number, zeroed on the stream before the launches
    uint32_t short_max;           // segments up to this length are sorted by one lane
};
// bytes of the scan's scratch (64-bit tile sums) for n counts
size_t listScanScratchBytes(uint32_t n);
// counts[0..n) -> offsets[0..n], offsets[n] = the total
int launchListScan(const uint32_t* counts, uint32_t n, unsigned long long* offsets, unsigned long long* tileSums, ihipStream_t* stream);
// sorts every segment by (t', global id) and resolves the records into the outputs
int launchListSort(const ListParams& q, ihipStream_t* stream);
// camera rays (camera_kernels.hip; crt_camera_rays*, crt_frame_guides*): the frames' rayGen for a w x h frame as n = w * h ray
// records {pos, kTMin, rayDirJ, kTMax}, record = py * width + px.  sample = kSampleCentre: the jitter (0.5, 0.5) of modes
// 0..100; else the two draws a mode-200 frame takes for (pixel, sample, seed)
constexpr uint32_t kSampleCentre = 0xFFFFFFFFu;
struct CameraRayParams {
    float pos[3];
    float rot[9];
    uint32_t width, height;
    uint32_t sample, seed;
    void* rays;                   // n records of 32 bytes, 16-byte aligned
};
int launchCameraRays(const CameraRayParams& p, ihipStream_t* stream);
// the edge-avoiding a-trous filter and its variance-guided form (denoise_kernels.hip; crt_denoise*, crt_denoise_variance*).
// Scratch: three float4 planes of width * height -- the guide plane {n.xyz, t} and two colour planes {c.rgb, v} that the passes
// ping-pong between; v >= 0: live (the variance; 0 for the plain filter), v = -1: not live
struct DenoiseParams {
    uint32_t width, height;
    uint32_t iterations;          // 1..8
    uint32_t demodulate;          // 0 / 1
    float sigma_first;            // the first term's scale.  Plain: 1 / sigma_color^2 of pass 0 (pass i: x 4^i); 0 switches the term off.
                                  // Variance: sigma_luminance as given (+inf switches the term off)
    float inv_sigma_normal2;      // 1 / sigma_normal^2
    float sigma_depth;            // as given (+inf switches the term off)
    const float* rgb;             // 3 floats per pixel
    const float* normal;          // 3
    const float* albedo;          // 3
    const float* t;               // 1
    const float* variance;        // 1; null: the plain filter
    float* out;                   // 3; may be rgb
    float* varianceOut;           // 1; may be variance; may be null
    void* guide;                  // scratch planes, 16 bytes per pixel each
    void* colour[2];
};
constexpr size_t kDenoiseScratchPerPixel = 48;
// pack, iterations - 1 passes, and the last pass fused with the multiply-back
int launchDenoise(const DenoiseParams& p, ihipStream_t* stream);
// temporal reprojection (temporal_kernels.hip; crt_temporal_accumulate*, crt_temporal_variance*): no scratch.  A history record
// is two float4 per pixel, {c.rgb, len} and {n.xyz, t}
struct TemporalParams {
    float posCur[3], rotCur[9];   // the camera of this frame
    float posPrev[3], rotPrev[9]; // the camera the history was taken with
    uint32_t width, height;
    uint32_t demodulate;          // 0 / 1
    uint32_t staticCamera;        // 1: the two cameras are equal bitwise, a pixel's history is its own record
    float alpha, depthTolerance, normalThreshold;
    float maxHistory;             // 1 .. 2^24, exact as a float
    const float* rgb;             // 3 floats per pixel
    const float* normal;          // 3
    const float* albedo;          // 3; may be null when demodulate == 0
    const float* t;               // 1
    const void* histPrev;         // null: no history
    void* histNext;
    float* out;                   // 3; may be rgb; may be null
    const float* prevPoint;       // crt_temporal_accumulate_motion*: 3 floats per pixel, a pixel's world point in the previous frame
                                  // (a non-finite component: not moved); null: the plain kernel
    // crt_temporal_variance*: luminance moments {m1, m2}, 2 floats per pixel, beside the history; all null: the kernels above
    const void* momPrev;          // null exactly when histPrev is
    void* momNext;
    float* variance;              // 1 float per pixel
    float alphaMoments;
    float minHistory;             // 1 .. 2^24, exact as a float
};
// the reprojection kernel and, when momNext is set, step V6 behind it: the variance from the records the first one wrote
int launchTemporal(const TemporalParams& p, ihipStream_t* stream);
// previous points of hits (motion_kernels.hip; crt_previous_points*, crt_frame_motion*): one lane per record, the triangle's
// vertices of the last snapshot weighted by the hit's barycentrics
struct PreviousPointsParams {
    const void* table;            // MeshEntry per mesh + terminator (mesh_table.hip.h)
    uint32_t nMeshes;
    uint32_t n;                   // records
    const float* world;           // 3 floats per vertex: the current world vertices
    const float* prev;            // those of the last snapshot; null: none was taken, every record is "not moved"
    const uint32_t* idx;          // 3 per triangle, mesh-local
    const uint32_t* inst;         // per record, as the ray queries write them
    const uint32_t* prim;
    const float* uv;              // 2 floats per record, 8-byte aligned
    float* point;                 // 3 floats per record
};
int launchPreviousPoints(const PreviousPointsParams& p, ihipStream_t* stream);
// gradients of the closest-hit and closest-point queries (grad_kernels.hip; crt_trace_rays_backward*, crt_closest_points_backward*):
// one lane per record, the triangle's current world vertices gathered as above, the vertex contributions added to `sums`
struct RayGradParams {
    const void* table;            // MeshEntry per mesh + terminator (mesh_table.hip.h)
    uint32_t nMeshes;
    uint32_t n;                   // records
    const float* world;           // 3 floats per vertex: the current world vertices
    const uint32_t* idx;          // 3 per triangle, mesh-local
    const float* rays;            // 8 floats per record, 16-byte aligned
    const uint32_t* inst;         // per record, as crt_trace_rays* writes them
    const uint32_t* prim;
    const float* t;
    const float* uv;              // 2 floats per record, 8-byte aligned
    const float* gradT;           // dL/dt per record; null: zeros
    const float* gradUv;          // dL/du, dL/dv per record, 8-byte aligned; null: zeros
    float* gradRays;              // 8 floats per record {dL/do, 0, dL/dd, 0}, 16-byte aligned; may be null
    double* sums;                 // 3 doubles per vertex, zeroed by the caller; null: no vertex gradient, no atomics
};
struct PointGradParams {
    const void* table;
    uint32_t nMeshes;
    uint32_t n;
    const float* world;
    const uint32_t* idx;
    const float* points;          // 4 floats per record, 16-byte aligned
    const uint32_t* inst;         // per record, as crt_closest_points* writes them
    const uint32_t* prim;
    const float* uv;
    const float* gradDist;        // dL/ddist per record
    float* gradPoints;            // 4 floats per record {dL/dp, 0}, 16-byte aligned; may be null
    double* sums;
};
int launchRayGrad(const RayGradParams& p, ihipStream_t* stream);
int launchPointGrad(const PointGradParams& p, ihipStream_t* stream);
// out[i] = float(sums[i]), n values: each float64 sum rounded once
int launchGradFinalize(const double* sums, float* out, size_t n, ihipStream_t* stream);
// exhaustive check of the triangle test's reciprocal (ray_kernels.hip rcpCheckKernel) into out[0..6] (device memory, zeroed
// except out[6] = ~0 by the caller)
int launchRcpCheck(unsigned long long* out, ihipStream_t* stream);

// device-side texture record (crt_texture with the pixel pointer replaced by an offset into the texel pool)
struct TextureRec {
    uint32_t type;
    float a[3], b[3];
    float scalar;
    uint32_t texel_offset, width, height, channels;
};

} // namespace crt
