// context.h — internal host-side state of a bh_ctx and the kernel launcher
// prototypes shared between the translation units of libbrush_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/brush_hip.h"
#include "../../include/brush_hip_lpips.h"
#include "../../include/brush_hip_image.h"
#include "../../include/brush_hip_exposure.h"
#include "../../include/brush_hip_bilagrid.h"
#include "../../include/brush_hip_depth_loss.h"
#include "../../include/brush_hip_normal_loss.h"
#include "../../include/brush_hip_distortion.h"
#include "../../include/brush_hip_mesh.h"
#include "../../include/brush_hip_features.h"
#include "../../include/brush_hip_feature_train.h"
#include "../../include/brush_hip_envmap.h"
#include "device_math.h"

namespace bh {

// Scratch arena: named slots that only ever grow, so the steady state of a
// training loop performs no hipMalloc/hipFree (the reference allocates ~20
// buffers per render, render.rs:104-268).
enum Slot : int {
    SLOT_COUNTERS = 0,       // 2 (ping-pong) x [COUNTER_SLOTS][2] u64: partial num_visible, num_intersections
    SLOT_DEPTH_KEYS,         // [N] u32 depth bits / sentinel
    SLOT_ISECT_COUNTS,       // [N] u32
    SLOT_MAX_RADIUS,         // [N] f32
    SLOT_SORT_KEYS_A,        // ping-pong buffers for the radix sort
    SLOT_SORT_KEYS_B,
    SLOT_SORT_VALS_A,
    SLOT_SORT_VALS_B,
    SLOT_SORT_HIST,          // digit totals | [nblocks][256] u32 block histograms (| the depth sort's digit bytes)
    SLOT_COMM_SCRATCH,       // direct all-reduce: the other ranks' versions of this rank's chunk (comm.hip)
    SLOT_BWD_CKPT,           // backward jobs: the forward blend's pixel-state checkpoints (rasterize.hip)
    SLOT_BWD_TOPLIST,        // ... and the bands' top-class job lists
    SLOT_SORT_PARTS,         // tile sort: per part [9][bins] pair counts (sort.hip tile_parts_*)
    SLOT_SCAN_SUMS,          // block sums for the scan
    SLOT_GLOBAL_FROM_COMPACT,
    SLOT_DEPTHS_SORTED,
    SLOT_CUM_TILES_HIT,
    SLOT_PROJECTED,
    SLOT_TILE_IDS,           // unsorted (tile, gid) pairs
    SLOT_ISECT_GIDS,
    SLOT_TILE_IDS_SORTED,
    SLOT_ISECT_GIDS_SORTED,
    SLOT_TILE_OFFSETS,
    SLOT_OUT_IMG,
    SLOT_VISIBLE,
    SLOT_V_COMBINED,
    SLOT_LOSS_MAP,
    SLOT_V_OUTPUT,           // [H,W,4]
    SLOT_GRADS,              // exchange buffer: visible | v_transforms | v_sh | v_raw_opac | v_refine
    SLOT_STATS,              // screen radius of the last train-step forward
    SLOT_LOSS_SCALAR,
    SLOT_MISC,
    SLOT_REFINE,             // refine plan: control block + 10 x [N] u32
    SLOT_REFINE_BOUNDS,      // percentile bounds: keys / sorted keys / indices
    SLOT_FOLDED_TRANSFORMS,  // train step with a 3D-filter floor: folded [N,10] / [N]
    SLOT_FOLDED_RAW_OPAC,
    SLOT_PLY_ROWS,           // PLY body being packed / unpacked
    SLOT_EXCH_BLOCKS,        // mask-keyed gradient exchange: per-block counts (+ total) / rank -> splat / compact rows
    SLOT_EXCH_IDX,
    SLOT_EXCH_COMPACT,
    SLOT_PROJECTED_BY_GID,   // [N,9] projected records at their splat id (visible splats only)
    SLOT_SLICE,              // depth-sliced forward: 8 control words (SLICE_CTRL_WORDS) | done bits [ceil(T/32)] | far tile offsets [T,2] | far group totals
    SLOT_SLICE_STATE,        // [H,W,4] raw blend state of the tiles the near slice left unsaturated
    SLOT_SLICE_COUNTS,       // [Nv] live-tile hits per far splat / their inclusive scan
    SLOT_SLICE_CUM,
    SLOT_NEAR_COUNTS,        // [N] tiles hit per splat at or in front of the tile's depth cut (per-tile cut lists)
    SLOT_TILE_ORDER,         // [8][ceil(T/8)] the forward blend's block -> tile map: every XCD band's tiles by descending forecast work
    SLOT_LOD_GRADS,          // bh_pup_accumulate_view: v_transforms [N,10] | v_sh [N,C,3] | v_raw_opac [N] | v_refine [N] (lod.hip)
    SLOT_LOD_FOLDED,         // ... and bh_eval_view: fold_min_scale(params): transforms [N,10] | raw_opac [N]
    SLOT_LOD_LOSS,           // ... dL/dimg [H,W,4] | the loss scalar
    SLOT_LOD_SORT,           // bh_decimate_to_count: keys [N] | sorted keys [N] | sorted ids [N]
    SLOT_KNN,                // bh_knn_log_scales: control | keys | sorted keys | order | rank cells [N] | x y z [N] | tree boxes (knn.hip)
    SLOT_EVAL,               // bh_eval_metrics: per-tile (squared error, SSIM) f64 partial sums (eval.hip)
    SLOT_LPIPS,              // bh_lpips_*: f64 partials | normalised inputs | scratch pair | activations of both images (lpips.hip)
    SLOT_PLY_COMPRESS,       // bh_splat_to_compressed_ply: box partials | box | Morton keys [N] | sorted keys [N] | row order [N] (ply_compress.hip)
    SLOT_IMAGE,              // bh_resize_u8: f32 intermediate | the two weight tables (image.hip)
    SLOT_DEPTH,              // launch_depth_backward: v_z [Nv] | the frame's accumulated depth [H,W] (depth.hip; nobody else looks inside: the backward hands v_z on)
    SLOT_POSE,               // bh_render_backward_pose_saved / bh_train_set_pose_grad: one f64 row of 12 per block of the pose pass (project.hip)
    SLOT_INTRINSICS,         // bh_render_backward_intrinsics_saved / bh_train_set_intrinsics_grad: one f64 row of 4 per block of the intrinsics pass (intrinsics.hip)
    SLOT_EXPOSURE,           // bh_exposure_backward: one f64 row of 12 per block of the exposure backward (exposure.hip)
    SLOT_CORRECTED,          // bh_train_step with an exposure or a bilateral-grid table (never both): [H,W,4] the exposed / sliced frame the loss reads (out_img stays as rendered)
    SLOT_PIXEL_LOSS,         // the pixel losses' partial sums, one f64 row of 4 per block (depth_loss.hip loss_partials): depth loss and metrics, normal consistency, distortion loss — one after another on the ctx stream, each followed at once by its final block
    SLOT_DEPTH_TERM,         // bh_train_step with a depth target or a normal term: expected depth [H,W] | v_depth [H,W] | the depth term's loss pair (4 floats)
    SLOT_NORMAL,             // bh_render_normal / launch_normal_backward: compact splat normals [Nv,3] | Vn [Nv,3] | the frame's accumulated normals [H,W,3] (normal.hip; the backward hands Vn on)
    SLOT_NORMAL_TERM,        // bh_train_step with a normal term: accumulated normals [H,W,3] | v_normal [H,W,3] | the term's loss pair (4 floats)
    SLOT_DISTORTION,         // bh_render_distortion / launch_distortion_backward: NDC depths m [Nv] | v_m (the term's own v_z) [Nv] | the frame's moment map [H,W,4] (distortion.hip)
    SLOT_DISTORTION_TERM,    // bh_train_step with a distortion term: the moment map [H,W,4] | the term's loss pair (4 floats)
    SLOT_BILAGRID,           // bh_bilagrid_backward: the train step's TV scalar (16 bytes) | the f64 gradient sums of the row | one f64 row of 48 per (unit, level) of the v_g pass (bilagrid.hip)
    SLOT_TSDF,               // bh_tsdf_extract[_count]: per sample the edge mask / triangle count / corner bits [n] | the vertex scan [n] | the triangle scan [n] (tsdf.hip)
    SLOT_FEATURES,           // bh_render_features / launch_feature_backward: compact features [Nv,C] | V [Nv,C] | the frame's accumulated feature map [H,W,C] (features.hip)
    SLOT_FEATURE_TERM,       // bh_train_step with a feature term: the feature map [H,W,C] | v_map [H,W,C] | the term's loss pair (4 floats)
    SLOT_FEATURE_GRAD,       // ... and its dense v_features [N,C], from the backward to the field's update
    SLOT_ENVMAP_FRAME,       // bh_train_step with an environment map: [H,W,4] the frame composited over the map (envmap.hip; out_img stays what K17 replays)
    SLOT_DEAL_REGION,        // depth sort, dealing K1 (depth_deal.h): [255][cap] (key, splat id) — the buckets K1 fills
    SLOT_SCENE,              // bh_splats_select_region with a count: one u32 per block of the select | the total (scene_edit.hip)
    SLOT_SPTSDF,             // sparse TSDF volumes (sparse_tsdf.hip): bh_sptsdf_commit: two bitmaps of the dilation [n_words] each | the words' bit counts [n_words]; bh_sptsdf_extract[_count]: as SLOT_TSDF, per allocated sample
    SLOT_COUNT
};

struct Buffer {
    void* ptr = nullptr;
    size_t cap = 0;
};

constexpr int MAX_PROF = 32;

// K1's block totals land in slot (block % COUNTER_SLOTS); the host adds the slots up after the readback
constexpr uint32_t COUNTER_SLOTS = 128;
// one counter set on the device:
//   [COUNTER_SLOTS][4] u64  visible, intersections, near intersections, near splats (K1's block totals; the last two only with
//                           per-tile depth cuts: the pairs the near pass will list and the splats that own them, see ViewState)
//   [COUNTER_SLOTS][2] u32  max depth key, max ~key over the visible splats: the key range the depth sort splits on.
// The first part is read back, the second stays on the device.
constexpr uint32_t COUNTER_K1_U64 = 4;                        // u64 words per slot of K1's block totals
constexpr size_t COUNTER_SET_BYTES = COUNTER_SLOTS * 8 * COUNTER_K1_U64 + COUNTER_SLOTS * 8;
constexpr uint32_t COUNTER_SET_U64 = (uint32_t)(COUNTER_SET_BYTES / 8);
constexpr uint32_t COUNTER_MINMAX_WORD = COUNTER_SLOTS * 2 * COUNTER_K1_U64;   // u32 index of the key-range part inside a set
// control words of SLOT_SLICE: [0] near-slice splats  [1] near pairs  [2] tiles the near pass left live  [3] far pairs
// [4] live column bands  [5] live row bands (32 bands per axis; the far pass skips splats whose box misses them)  [6..7] spare
constexpr uint32_t SLICE_CTRL_WORDS = 8;
// Both radix sorts (sort.hip, depth_sort.hip): histogram blocks per group total.  A scatter block adds up the totals of the groups in
// front of its own and the histograms of the earlier blocks of its own group: no scan launch between histogram and scatter.
constexpr uint32_t SORT_GROUP_BLOCKS = 32;
constexpr uint32_t FAR_GROUP_BLOCKS = 64;   // far slice: count-kernel blocks per group total (<= the projection workgroup size)
constexpr size_t COUNTER_READ_BYTES = COUNTER_SLOTS * 8 * COUNTER_K1_U64;
// ... or, when the depth sort's first kernel adds the slots up on the device: [COUNTER_K1_U64] u64 totals
constexpr uint32_t HOST_SUM_WORDS = 2 * COUNTER_K1_U64 + 1;   // (+ the tag word the host polls)
constexpr uint32_t HOST_DEAL_WORD = HOST_SUM_WORDS;           // ... and behind it: != 0, K1's deal overflowed a bucket (depth_deal.h), the order is not there yet
// pinned host block: [16] u32 scalars (refine control block / bounds picks / exchange rows) | the counter slots | the loss word.
// The loss has a word of its own BEHIND everything the refine / bounds / exchange readbacks overwrite.
constexpr size_t HOST_LOSS_WORD = 16 + COUNTER_READ_BYTES / 4;
constexpr size_t HOST_GATE_WORD = HOST_LOSS_WORD + 16;   // depth-sliced forward: tiles the near slice left unsaturated
constexpr size_t HOST_GATE_TAG_WORD = HOST_GATE_WORD + 1;   // ... and the tag the kernel queued BEHIND the near blend stores when it starts (= the blend has finished)
constexpr size_t HOST_COUNTERS_BYTES = 64 + COUNTER_READ_BYTES + 64 + 64;

struct Profiler {
    int level = 0;  // 0 off, 1 every stage, 2 only the dominant kernel (2 events per step)
    const char* names[MAX_PROF];
    float ms[MAX_PROF];
    uint32_t calls[MAX_PROF];
    int count = 0;
    // pending (start, stop) event pairs, resolved lazily at fetch / sync time
    struct Pending { int idx; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    // level 2: the dominant kernel's launch carries its own (start, stop) events (hipExtLaunchKernelGGL): the times
    // come from the dispatch packet itself, without the two barrier packets (~5.6 us of bubble each) that
    // hipEventRecord puts in front of and behind the kernel
    hipEvent_t ext_a = nullptr, ext_b = nullptr;
};

// Per-view state of the per-tile depth cut (BH_FLAG_SLICED_LISTS, automatic mode; api.hip has the whole story, lists.hip the policy): for every tile the
// depth key behind which the tile needed no splat the last time THIS view was rendered (+ a margin), 0xFFFFFFFF = list everything.
// Written in place by the blend kernel of every forward of the view, read by K1 / K5 / the far pass of its next one.
// Bit 0 of an entry is not part of the cut: K1 sets it when it meets a pair BEHIND the cut ("this tile's near list is incomplete
// this frame"), the blend kernel reads it and rewrites the entry with the bit clear.  Cuts are compared without it (zcut_near).
constexpr uint32_t ZCUT_ALL = 0xFFFFFFFEu;
BH_DEV bool zcut_near(uint32_t key, uint32_t cut) { return (key >> 1) <= (cut >> 1); }
struct ViewState {
    uint32_t* zcut = nullptr;       // [tile_bw * tile_bh] device; directly behind it: work[tile_bw * tile_bh], the splats every tile blended at the
                                    // view's last frame (the forward blend's tile order, rasterize.hip); behind that: [VIEW_SPL_WORDS] the depth
                                    // sort's splitter tables of the view
    uint32_t tile_bw = 0, tile_bh = 0;
    bool seeded = false;            // a forward of this view has written the table
    uint32_t exact_frames = 0;      // frames to render with complete lists before the cut is trusted again (the forecast kept failing)
    uint32_t penalty = 0;           // one bit per recent cut frame: its far pass had to run (lists.hip view_outcome)
    uint64_t last_used = 0;         // LRU stamp (the ctx's forward counter at the view's last frame)
    uint32_t gap = 0;               // forwards between the view's last two frames (a new view: the number of views the ctx knows) —
                                    // how stale the table will be when it is next read: the margin written into it grows with it
    uint32_t last_pairs = 0;        // num_intersections of the view's last frame
    uint32_t complete_frames = 0;   // frames to render with complete lists because cutting saved (almost) nothing last time; then one probe frame
    bool spl_written[2] = {false, false};   // the view's depth-sort splitter tables ([0] complete lists, [1] cut lists) have been written by a frame
    uint32_t spl_keys[2] = {0, 0};          // ... and the listed splats of the frame that wrote each last (>= SPL_MIN_KEYS: the table holds quantiles — K1 may deal by it)
    bool casual = false;            // created by a forward-only frame keyed by its camera (a viewer / eval render): these compete for CASUAL_VIEW_STATES tables only
};
constexpr uint32_t CUT_MIN_PAIRS = 1500000u;   // frames with fewer pairs keep complete lists (nothing to save)
// work classes of the blend backward's longest-first order (rasterize.hip): counters [8 XCD bands][LPT_CLASSES] behind the tile table
constexpr uint32_t LPT_CLASSES = 64;
constexpr uint32_t LPT_HEADER_WORDS = 8 * LPT_CLASSES + 64;   // the counters + 64 control words ([0]: checkpoint slots handed out), cleared with the tile table
// Backward JOBS (round 6, rasterize.hip): the blend backward's unit of work is not a tile but a segment of BWD_SEG entries of a
// tile's blended list.  The forward blend leaves the pixel state (colour so far, signed transmittance) of its 256 pixels at every
// segment boundary — a CHECKPOINT, 4 KB — and files one job per segment; a job starts from its checkpoint instead of replaying
// the tile from its first splat.  The launch then lasts as long as its total work, not as long as its heaviest tile.
constexpr uint32_t BWD_SEG = 128;       // list entries per job (two staging batches)
constexpr uint32_t BWD_MAX_SEGS = 64;   // checkpointed segments per tile; a tile's last job takes whatever lies behind
struct BwdJobs {                        // all zero: one job per tile (far-sliced frames, option bwd_jobs = 0)
    float4* ckpt = nullptr;             // [ckpt_cap][4][64] pixel state at a segment's first entry.  Slot of (tile, segment s >= 1) =
                                        // (first list entry of the tile) / BWD_SEG + tile + s - 1: unique without an atomic or a table, because the
                                        // tiles' lists lie one behind the other (< listed pairs / BWD_SEG + tiles slots; a slot >= ckpt_cap does not exist:
                                        // that tile keeps the rest of its list as one job)
    uint32_t ckpt_cap = 0;
    uint32_t* top_list = nullptr;       // [8][top_cap] the bands' TOP class (every full segment lands there: more entries than tiles)
    uint32_t top_cap = 0;
};
// XCD BANDS.  The dispatcher deals consecutive workgroups to the eight XCDs in turn, so block b of a blend launch runs on XCD b & 7 and
// takes the (b >> 3)-th tile of BAND b & 7.  band_mode 0: a band is a contiguous eighth of the tile index range (whole tile rows: the
// XCD's L2 sees one spatially coherent strip of the frame).  band_mode 1 (round 6): bands are dealt in chunks of BAND_CHUNK horizontally
// adjacent tiles, chunk c to band c & 7 — every XCD gets an even share of any frame (an object in front of an empty background leaves
// the top and bottom strips with nothing to do: two of eight XCDs idle through both blend kernels, and the object's heaviest tiles
// share the L2 and the SIMDs of two others).  Every band has band_slots() slots; a slot may name no tile (>= num_tiles).
constexpr uint32_t BAND_CHUNK = 4;   // (2 / 4 / 8 / 16 measured: profiles/EXPERIMENTS.md)
inline __host__ __device__ uint32_t band_slots(uint32_t num_tiles) {
    const uint32_t p = (num_tiles + 7u) / 8u;
    return ((p + BAND_CHUNK - 1u) / BAND_CHUNK) * BAND_CHUNK;
}
inline __host__ __device__ uint32_t band_tile(uint32_t band, uint32_t i, uint32_t per, uint32_t mode) {
    return mode ? ((i / BAND_CHUNK) * 8u + band) * BAND_CHUNK + (i % BAND_CHUNK) : band * per + i;
}
// block -> tile of the window, for every blend launch of band_slots() * 8 blocks (>= num_tiles: the slot names no tile)
BH_DEV uint32_t tile_of_block(uint32_t b, uint32_t num_tiles, uint32_t band_mode) {
    const uint32_t per = band_slots(num_tiles);
    const uint32_t i = b >> 3;
    return i < per ? band_tile(b & 7u, i, per, band_mode) : 0xFFFFFFFFu;
}
// SPLIT TILES (round 6, rasterize.hip): the forward blend cannot be cut along a tile's list (a pixel's stop rule needs everything in
// front of it), so a launch lasts as long as its heaviest tile — one wave working through its list at a lone wave's pace.  The few
// tiles whose forecast work (the view's last frame) is several times their band's mean are blended by FOUR waves, one per 8 x 8 pixel
// quadrant (four independent one-wave blocks; the last of them to finish does the tile's bookkeeping).  K1's order blocks decide which:
// the first split_count[band] ranks of a band's descending order.  Layout behind the order table [8][per]:
//   split_count[8] | split_scratch[8][SPLIT_MAX][4] = finished quadrants | max last useful entry | max entry reached | 1 = a quadrant is unsaturated
constexpr uint32_t SPLIT_MAX = 128;         // split tiles per XCD band at most (the grid carries 3 * SPLIT_MAX extra blocks per band)
constexpr uint32_t SPLIT_MIN_WORK = 256;    // a tile below this many blended splats is never split
constexpr uint32_t SPLIT_TAIL_WORDS = 8u + 8u * SPLIT_MAX * 4u;
constexpr uint32_t BWD_CKPT_MAX_SLOTS = 96u * 1024u;   // 384 MB of checkpoints at most (frames with > ~11 M listed pairs split only their first tiles)
constexpr uint32_t DSORT_SPL_STRIDE = 260;            // words of one depth-sort splitter table (depth_sort.hip SPLITTERS)
constexpr uint32_t VIEW_SPL_WORDS = 2 * DSORT_SPL_STRIDE;   // a view keeps two behind its tile table: [0] frames with complete lists, [1] cut lists
// DEALING K1 (depth_deal.h): K1 puts every listed splat straight into its depth-sort bucket.  One counter set: 255 bucket words
// (low half: splats, high half: their tile counts) and the overflow word, each in a 128-byte line of its own; two sets, K1 clears the idle one.
constexpr uint32_t DEAL_BUCKETS = 255;
constexpr uint32_t DEAL_LINE_U64 = 16;
constexpr uint32_t DEAL_SET_U64 = (DEAL_BUCKETS + 1u) * DEAL_LINE_U64;
constexpr uint32_t DEAL_OVERFLOW_U64 = DEAL_BUCKETS * DEAL_LINE_U64;
struct DealArgs {                                // all NULL: K1 does not deal
    const uint32_t* spl = nullptr;               // the view's splitter table of this list mode (depth_sort.hip SPLITTERS)
    unsigned long long* ctr = nullptr;           // [DEAL_SET_U64] this frame's counter set (zero on entry)
    uint2* region = nullptr;                     // [DEAL_BUCKETS][cap] (key, splat id) in arrival order
    uint32_t cap = 0;                            // slots per bucket; a splat that finds none sets the overflow word
};
constexpr size_t MAX_VIEW_STATES = 4096;
constexpr uint64_t DIRECT_ALLREDUCE_MIN_FLOATS = 1u << 16;   // shorter messages are latency-bound: ncclAllReduce
constexpr uint32_t AUTO_EXACT_FRAMES = 12;   // frames a view renders complete lists after a cut frame that listed > auto_exact_share of its pairs
// Forward-only frames that name no view (a viewer's free camera, an eval render, a pose-optimised camera: a new hash every frame) get
// a table only when the same camera is seen a SECOND time, and at most this many of them are kept: such frames cut nothing, the table
// only orders their blend's tiles.
constexpr size_t CASUAL_VIEW_STATES = 32;
constexpr size_t SEEN_KEYS = 64;   // ring of camera hashes met once
constexpr size_t VIEW_TABLE_BYTES = (size_t)256 << 20;   // ... and at most this much device memory in tables (8 B per tile and view: 64 KB at 1080p, 253 KB at 4K)

// scratch of a depth-sliced forward (rasterize.hip SliceArgs)
struct RasterSlice {
    uint32_t* done_bits = nullptr;
    uint32_t* unsat_count = nullptr;
    uint32_t* gate_host = nullptr;   // pinned host word: the near pass stores 1 there when it parks a tile (the host's copy of unsat_count != 0)
    float* state = nullptr;
    const uint32_t* offsets_near = nullptr;
    // per-tile depth cut: the view's table (read: is the tile's near list complete?  written: what the tile needed this time),
    // the depth keys in compact order and their number (to turn "last useful splat + margin" into a key); cut_active: the lists of
    // this frame were built against the table (else it is only written)
    uint32_t* zcut = nullptr;
    const uint32_t* depth_keys_sorted = nullptr;
    uint32_t nv = 0;
    bool cut_active = false;
    uint32_t* live_bands = nullptr;   // the two band words of the slice table (SLICE_CTRL_WORDS): sliced phases only
    uint32_t* work = nullptr;              // [T] the view's per-tile blended counts: written by every phase that finishes a tile
    const uint32_t* order = nullptr;       // [8][ceil(Tw/8)] block -> local tile of this launch (K1 sorted each XCD band by the view's last work), or NULL
    uint32_t order_mode = 1;
    uint32_t* split = nullptr;        // split tiles: split_count[8] | split_scratch (behind `order`; written by K1's order blocks), or NULL
    uint32_t margin_pct = 150;        // depth-order margin behind a tile's last useful splat, in % of its rank
    BwdJobs jobs{};                   // BWD_INFO: file the backward's work as jobs with checkpoints (ckpt != NULL)
};

// One forward call: bh_render_forward's arguments, or the train step's, with where the train step wants its outputs and clears.
// forward_impl reads the call's settings from here only (the ctx holds options and what outlives the call).
struct ForwardRequest {
    BhCamera cam{};
    uint32_t n = 0, sh_degree = 0, flags = 0;
    const float* transforms = nullptr;
    const float* sh_coeffs = nullptr;
    const float* raw_opacities = nullptr;
    float bg[3] = {0, 0, 0};
    uint32_t view_id = 0;              // keys the per-view table (lists.hip view_key; 0: the camera does)
    float* visible = nullptr;          // train step: visible / max_radius land here (its stats buffer), else in the arena
    float* max_radius = nullptr;
    size_t visible_floats = 0;         // floats to clear at `visible` (its section of the exchange buffer incl. padding; 0: n)
    float* grad_begin = nullptr;       // train step: a gradient span K1 zero-fills on its way (GradClears)
    size_t grad_floats = 0;
    bool defer_decision = false;       // return with far_job.pending instead of waiting for the near pass's gate word (bh_train_step)
    bool allow_cut = true;             // false: complete lists whatever the view's table says (the second attempt, finish_far_slice)
};

// The working set of one forward: what forward_impl computes once per call and its later stages read — its own list build and
// blend, and the far slice if the frame needs one (a FarJob holds a copy).
struct Frame {
    ViewUniforms u{};
    float bg[3] = {0, 0, 0};
    bool bwd_info = false, smooth = false;
    uint32_t nv = 0, ni = 0, budget = 0, num_tiles = 0, tile_bits = 0;
    float* proj_by_gid = nullptr;
    uint32_t* gfc = nullptr;
    float* projected = nullptr;
    uint32_t* cum = nullptr;
    uint32_t* slice_info = nullptr;
    uint32_t* done_bits = nullptr;
    uint32_t* tile_offsets_far = nullptr;
    uint32_t* far_counts = nullptr;
    uint32_t* far_block_totals = nullptr;
    uint32_t* far_group_totals = nullptr;   // zeroed by K1 with the slice table
    uint32_t* tile_ids = nullptr;
    uint32_t* isect_gids = nullptr;
    uint32_t* tile_ids_sorted = nullptr;
    uint32_t* isect_gids_sorted = nullptr;
    float* out_f32 = nullptr;
    uint32_t* out_u8 = nullptr;
    float* visible = nullptr;
    uint32_t* lpt = nullptr;   // longest-first tile order of a BWD_INFO forward (rasterize.hip), or NULL
    float class_width = 8.0f;
    RasterSlice rs{};
};

// The far slice of a depth-sliced forward, ready to be queued: everything launch_* needs (lists.hip enqueue_far_slice).
struct FarJob {
    bool pending = false;   // the near slice is queued and its gate word is on its way to the host; the far slice is undecided
    Frame frame{};
    // how the host learns that the near blend has finished: an event behind it (recorded when the job is created, or late, by
    // finish_far_slice), or — bh_train_step — the tag word its loss kernel stores when it starts (no event: a barrier packet
    // costs ~6 us of bubble in front of the next kernel)
    bool gate_event_recorded = false;
    uint32_t gate_tag = 0;
    // per-tile cut lists: only the splats with a pair in front of some cut were sorted and listed, so there is no far pass — if a
    // tile is still live behind a cut list the forecast has failed and the whole forward is run again with complete lists
    // (lists.hip finish_far_slice): the request to replay
    bool by_cut = false;
    ViewState* view = nullptr;      // whose prediction failed
    bool view_shared = false;       // ... and whether that is the table of view id 0 (shared by all frames without an id)
    ForwardRequest req{};
};

// Clears done "on the way" by a forward's kernels, and how the train step wants its gradient span treated.
//   span:  NONE        nobody cleared the span: the backward zero-fills every dense output it writes into
//          ZEROED      K1 of forward `generation` cleared the WHOLE ext span it was given (exchange / multi-GPU step)
//          ROW_MARKS   single-GPU train step: only the refine-weight vector is clear (K1 or a fill did it); K18 marks the rows it
//                      writes in that vector's sign bits and the update kernel reads exactly those rows — the backward must NOT
//                      fill the span and must run K18 in marking mode
//   accum: K5 of forward `generation` cleared v_combined [num_listed_splats, 10]
// Transitions: begin_forward() -> (k1_cleared_span | k5_cleared_accum)* -> stamp(generation) -> [mark_rows()] -> take_*() in the
// backward of THAT generation (anything else finds NONE / false).  A backward always leaves the record empty: the accumulator
// and the span are dirty afterwards.
struct GradClears {
    enum Span : uint8_t { NONE = 0, ZEROED, ROW_MARKS };
    Span span = NONE;
    bool accum = false;
    uint64_t generation = 0;   // 0: not stamped yet (the forward is still being queued)
    void begin_forward() { span = NONE; accum = false; generation = 0; }
    void k1_cleared_span() { span = ZEROED; }
    void k5_cleared_accum(bool yes) { accum = yes; }
    void stamp(uint64_t gen) { generation = gen; }
    // train step, single GPU: the refine-weight vector is clear (by K1: span == ZEROED for that sub-span, or by the caller's fill)
    void mark_rows() { span = ROW_MARKS; }
    bool valid_for(uint64_t gen) const { return generation != 0 && generation == gen; }
    Span take_span(uint64_t gen) { const Span s = valid_for(gen) ? span : NONE; span = NONE; return s; }
    bool take_accum(uint64_t gen) { const bool a = valid_for(gen) && accum; accum = false; return a; }
};

// What a backward needs of the forward it belongs to (RenderBackwards' saved state, bwd/burn_glue.rs:336-371): the host side of it.
struct ForwardState {
    BhRenderOut out{};
    ViewUniforms uniforms{};
    uint32_t n = 0, sh_degree = 0, flags = 0;
    float bg[3] = {0, 0, 0};
    uint32_t* lpt = nullptr;   // longest-first tile order of the forward (rasterize.hip), or NULL
    BwdJobs jobs{};            // ... filed as jobs with checkpoints (ckpt != NULL), or as whole tiles
};
// A forward whose arena blocks were detached from the ctx (bh_render_retain): it stays replayable while later forwards run.
constexpr int RETAIN_SLOTS = 14;
struct Retained {
    ForwardState fs;
    Buffer blocks[RETAIN_SLOTS];
};

// The depth term of a backward (depth.hip, brush_hip_depth.h): <v_depth, depth map `mode` of the forward>
struct DepthTerm {
    const float* v_depth = nullptr;   // [H,W]
    uint32_t mode = 0;                // BH_DEPTH_ACCUMULATED or BH_DEPTH_EXPECTED
};

// The normal term of a backward (normal.hip, brush_hip_normal.h): <v_normal, normal map `mode` of the forward>
struct NormalTerm {
    const float* v_normal = nullptr;   // [H,W,3]
    uint32_t mode = 0;                 // BH_NORMAL_ACCUMULATED or BH_NORMAL_UNIT
};

struct ParamTable;   // param_table.h: the host core of bh_exposure, bh_bilagrid and bh_envmap

// The distortion term of a backward (distortion.hip, brush_hip_distortion.h): <v_distortion, dist of the forward>
struct DistortionTerm {
    const float* v_distortion = nullptr;   // [H,W], or NULL: the uniform cotangent `gain` at every pixel
    float gain = 0.0f;
    uint32_t kind = 0;                     // BH_DISTORTION_Z or BH_DISTORTION_NDC
    float near_z = 0.0f, far_z = 0.0f;     // NDC only
    const float* moments = nullptr;        // [H,W,4] the frame's moment map if the caller has rendered it (the train step), or NULL
};

// The feature term of a backward (features.hip, brush_hip_features.h): <v_map, feature map of `features`>
struct FeatureTerm {
    const float* features = nullptr;   // [N,C] by global splat id
    uint32_t channels = 0;             // 1 .. BH_FEATURE_MAX_CHANNELS
    const float* v_map = nullptr;      // [H,W,C]
    float* v_features = nullptr;       // [N,C] out: dense, fully overwritten
    // what the caller has already produced for this frame (the train step), or NULL: the backward gathers and blends its own
    const float* map_acc = nullptr;    // [H,W,C] the frame's accumulated feature map
    const float* compact = nullptr;    // [Nv,C] the compact rows behind it, at feature_term_rows' address
};

// One backward on a saved forward (api.hip backward_impl): the parameters the forward rendered, where the gradients go, and the
// terms beside the colour term's <v_output, image>.
struct BackwardCall {
    const float* transforms = nullptr;
    const float* sh_coeffs = nullptr;
    const float* raw_opacities = nullptr;
    float* v_transforms = nullptr;
    float* v_sh_coeffs = nullptr;
    float* v_raw_opacities = nullptr;
    float* v_refine_weight = nullptr;
    size_t span_floats = 0;        // != 0 (the train step): the four outputs are one span of that many floats from v_transforms on
    bool want_refine = true;       // false: nobody reads the refine weight
    const DepthTerm* depth = nullptr;             // its raw sums join the accumulator between K17 and K18, its v_z lands behind K18
    const NormalTerm* normal = nullptr;           // likewise, behind depth's; its Vn lands behind depth's v_z
    const DistortionTerm* distortion = nullptr;   // likewise, behind normal's; its v_z joins depth's or goes through the same scatter
    const FeatureTerm* feature = nullptr;         // likewise, behind distortion's; its V lands in v_features behind the other scatters
    float* v_viewmat = nullptr;    // [12] (brush_hip_pose.h): the pose pass runs behind K18 on the rows it left in v_combined
    float* v_intrinsics = nullptr; // [4] (brush_hip_intrinsics.h): the intrinsics pass, behind the pose pass on the same rows
};

// What is attached to the train steps of a ctx: the bh_train_set_* calls write here, plan_step (train.hip) reads it.  A term counts for
// a step when its accessor says so; everything else about it is the step's business.
struct StepTerms {
    const bh_lpips* lpips = nullptr;  // bh_train_set_lpips: the step adds lpips_weight * LPIPS (lpips.hip); NULL or 0 = off
    float lpips_weight = 0.0f;
    float* pose_grad = nullptr;       // bh_train_set_pose_grad: the step writes its v_viewmat [12] here (brush_hip_pose.h); NULL = off
    float* intrinsics_grad = nullptr; // bh_train_set_intrinsics_grad: the step writes its v_intrinsics [4] here (brush_hip_intrinsics.h); NULL = off
    bool depth_attached = false;      // bh_train_set_depth: the step adds the depth term of depth_target (brush_hip_depth_loss.h); weight <= 0 = off
    BhDepthTarget depth_target{};
    bool normal_attached = false;     // bh_train_set_normal: the step adds the normal-consistency term (brush_hip_normal_loss.h); weight <= 0 = off
    BhNormalTermConfig normal_term{};
    bool distortion_attached = false; // bh_train_set_distortion: the step adds the distortion term (brush_hip_distortion.h); only ever true with a weight > 0
    BhDistortionTermConfig distortion_term{};
    bool feature_attached = false;    // bh_train_set_features: a field is attached (brush_hip_feature_train.h); feature_field.step counts its updates
    BhFeatureField feature_field{};
    BhFeatureTarget feature_target{}; // ... and the target of the next steps; weight <= 0 (or not a number, or no target): no term
    bh_exposure* exposure = nullptr;  // bh_train_set_exposure: the step exposes its frame with the row of the batch's view and updates it; NULL = off
    bh_bilagrid* bilagrid = nullptr;  // bh_train_set_bilagrid: the step slices its frame with the grid of the batch's view and updates it; NULL = off
    float bilagrid_tv_weight = 0.0f;  // ... and adds this much of the grid's total variation to the loss
    bh_envmap* envmap = nullptr;      // bh_train_set_envmap: the step composites its frame over the map before the loss and updates the map; NULL = off

    bool lpips_on() const { return lpips != nullptr && lpips_weight > 0.0f; }
    bool depth_on() const { return depth_attached && depth_target.weight > 0.0f; }
    bool normal_on() const { return normal_attached && normal_term.weight > 0.0f; }
    bool distortion_on() const { return distortion_attached; }
    bool feature_on() const { return feature_attached && feature_target.weight > 0.0f; }
};

}  // namespace bh

// The blend backward accumulates RAW per-splat sums into v_combined and the projection backward maps them to the reference's
// RasterizeGrads row (and stores it back) — rasterize.hip / project.hip.

struct bh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string last_error;
    bh::Buffer slots[bh::SLOT_COUNT];
    uint32_t* host_counters = nullptr;  // pinned, HOST_COUNTERS_BYTES
    hipEvent_t readback_ev = nullptr;   // marks the count readback of the forward (the depth sort is queued behind it)
    hipEvent_t gate_ev = nullptr;       // depth-sliced forward: the near slice's blend + the copy of its gate word have run
    bool counters_ready = false;        // the counter pair the next forward accumulates into is known to be zero
    uint32_t counter_phase = 0;         // which half of SLOT_COUNTERS that is
    // state of the last forward (what RenderBackwards saves, bwd/burn_glue.rs:336-371)
    bool have_forward = false;
    bh::ForwardState latest;          // complete only while have_forward (forward_impl fills it at its end)
    uint64_t generation = 0;          // stamped into every BhRenderOut a forward of this ctx returns (bh_render_backward_saved checks it)
    std::vector<bh::Retained> retained;   // forwards detached by bh_render_retain, until bh_render_release
    std::vector<bh::Buffer> pool;     // blocks given back by bh_render_release: ensure() takes from here before it asks hipMalloc
    // What the forward's kernels cleared on their way, so that the backward can skip its fills (K1: the train step's gradient span;
    // K5: the backward's accumulator v_combined).  ONE record with explicit transitions (bh::GradClears below) instead of loose
    // flags: every fact is tied to the forward (generation) whose kernels established it and is consumed exactly once.
    bh::GradClears clears;
    float* pending_loss_dst = nullptr; // where bh_sync delivers the last step's loss
    void* image_tab_host = nullptr;   // bh_resize_u8: pinned staging of the weight tables (image.hip) ...
    size_t image_tab_cap = 0;
    hipEvent_t image_tab_ev = nullptr; // ... free again once this event (behind their copy) has completed
    bh::StepTerms terms;              // what the bh_train_set_* calls attached to the next train steps (train.hip)
    std::vector<bh::ParamTable*> param_tables;   // every learned table of this ctx, of any kind (param_table.h): bh_destroy frees what is left
    void* comm = nullptr;             // RCCL communicator (comm.hip), or NULL
    // the library communicator's side stream: the mask-keyed exchange sums the visible flags and lists their union there,
    // beside the backward on the ctx stream (train.hip); comm_ev marks "the forward is done" for it
    hipStream_t comm_stream = nullptr;
    hipEvent_t comm_ev = nullptr;
    int comm_rank = 0, comm_world = 1;
    // depth-sliced lists (BH_FLAG_SLICED_LISTS): share of the pair list the near slice takes.  <= 0: automatic, per-tile depth
    // cuts from the view's last frame (bh_set_list_slicing)
    float slice_fraction = 0.0f;
    float last_slice_share = 1.0f;    // what the last sliced forward used (1 = one slice = the exact lists); diagnostics
    // The far slice costs ~12 launches even when every one of them is a no-op (~4.5 us each on this chip), so whether to queue
    // it is decided on the HOST where possible: far_direct = the previous sliced frame needed it -> queue it right away
    // (device-gated, no host wait; the gate word is copied out to keep learning); otherwise the host reads the gate word —
    // bh_render_forward waits for it, bh_train_step queues the loss kernels first and waits behind them (far_job.pending).
    bool far_direct = false;
    uint32_t readback_tag = 0;        // tag of the last count readback the host polled for (depth_sort.hip counter_sums_to_host)
    uint32_t gate_tag = 0;            // tag of the last deferred far-slice decision
    bool gate_signal_queued = false;  // a kernel that stores far_job.gate_tag when it starts is queued behind the near blend
    bool gate_learn = false;          // a gate word copied out by a far_direct frame has not been looked at yet
    uint32_t far_launches = 0;        // diagnostics: sliced forwards that queued a far slice / had to be run again with complete lists
    // per-tile depth cuts (automatic slicing): one table per view id (bh_set_view_id / BhTrainBatch.view_id; 0 = the ctx's own slot)
    // keyed by the caller's view id, or — id 0 — by a hash of the camera (lists.hip view_key): an unmodified SplatTrainer::step
    // (train.rs:176: a SceneBatch carries no view index, brush-dataset/src/scene.rs:138-147) gets the same tables
    std::unordered_map<uint64_t, bh::ViewState> views;
    uint64_t seen_keys[bh::SEEN_KEYS] = {};   // camera hashes of forward-only frames that found no table (lists.hip view_state)
    uint32_t seen_pos = 0;
    uint32_t casual_views = 0;                // tables whose ViewState::casual is set
    uint32_t view_id = 0;             // bh_set_view_id: the view id of the caller's bh_render_forward calls
    uint64_t view_clock = 0;
    // The margin behind a tile's last useful splat adapts (lists.hip cut_margin_pct): x (gap / 2)^(1/3) for a view that comes back
    // after `gap` frames, x margin_scale — multiplied by 1.5 when a forecast fails, by 0.998 when one holds (about one second
    // attempt in 200 cut frames at equilibrium), within [0.5, 16].  A scene that still moves fast (early training, many views between
    // two visits) gets deep margins, a settled one tight ones.
    float margin_scale = 1.0f;
    float ctrl_up = 1.5f, ctrl_down = 0.998f, ctrl_floor = 0.5f, ctrl_gap_exp = 1.0f / 3.0f;   // BH_CUT_CTRL="up:down:floor:gap_exp" (A/B)
    uint32_t cut_min_pairs = bh::CUT_MIN_PAIRS;   // bh_set_list_cut_threshold / BH_CUT_MIN_PAIRS
    bool knob_spec_k5 = true;             // option spec_k5: K5 queued in front of the count readback (api.hip)
    bool knob_event_waits = false;        // BH_EVENT_WAITS (A/B): the host's two mid-step waits use events behind the kernels, as before round 5, instead of polled tag words
    bool knob_readback_copy = false;      // BH_READBACK_COPY (A/B): counts and gate word reach the host through copy launches as before round 4
    bool knob_no_view_hash = false;       // BH_NO_VIEW_HASH (A/B): frames without a view id share ONE table (rounds 4's behaviour) instead of being keyed by their camera
    bool knob_fixed_margin = false;       // BH_CUT_MARGIN_FIXED (A/B): the margin is BH_CUT_MARGIN_PCT for every frame (rounds 4's behaviour), not adaptive
    bool knob_cut_sort_all = false;       // BH_CUT_SORT_ALL (A/B): with per-tile cuts, still sort every visible splat
    uint32_t feature_chunk = 0;           // option feature_chunk: channels per pass of the feature-map blends (features.hip); 0: feature_chunk(C)
    uint32_t knob_band_mode = 1;          // XCD bands of the blend kernels: 0 contiguous eighths of the tile range, 1 dealt in chunks of 8 tiles
    uint32_t knob_k16_waves = 0;          // forward blend: resident waves per SIMD (0 / 8: all eight; fewer: later tiles are dispatched as earlier ones finish)
    uint32_t knob_k16_split = 250;        // forward blend: split tiles at >= max(SPLIT_MIN_WORK, this / 100 x the band's mean forecast work); 0: never
    uint32_t knob_k16_split_min = bh::SPLIT_MIN_WORK;
    uint32_t knob_k16_split_of_max = 45;  // ... and this many percent of the band's heaviest tile
    const uint32_t* last_split = nullptr; // (test-hooks build: bh_debug_split_counts) the last forward's split counts, or NULL
    uint32_t knob_k16_order = 1;          // BH_K16_ORDER: 0 index order, 1 by the view's last per-tile work (descending), 2 dealt (A/B)
    uint32_t knob_cut_margin_pct = 150;   // BH_CUT_MARGIN_PCT: margin behind a tile's last useful splat, % of its depth rank (A/B)
    bh::FarJob far_job;
    uint32_t refine_n = 0, refine_new_n = 0;  // a bh_refine_plan awaiting its bh_refine_apply
    bool dsort_deal_lds_raised = false;   // ... and dsort_deal_bucket_kernel
    bool dsort_lds_raised = false;    // likewise dsort_bucket_kernel (depth_sort.hip)
    // the sorts' group tables (sort.hip SortGroups): two sets of sort_groups_cap words; set sort_groups_cur is all zero, the other one
    // holds the last sort's sums in its first sort_groups_dirty words
    uint32_t* sort_groups = nullptr;
    size_t sort_groups_cap = 0, sort_groups_dirty = 0;
    uint32_t sort_groups_cur = 0;
    uint32_t* dsort_spl = nullptr;    // [DSORT_SPL_STRIDE] device: the depth sort's splitter table (depth_sort.hip SPLITTERS) of frames without a view
    bool dsort_spl_written = false;   // a frame has written it (until then a frame sorts a sample first)
    uint32_t dsort_spl_keys = 0;      // ... and the listed splats of the frame that wrote it last (ViewState::spl_keys)
    unsigned long long* deal_ctr = nullptr;   // [2][DEAL_SET_U64] device: the dealing K1's counter sets (depth_deal.h); every K1 launch clears the idle one
    uint32_t deal_phase = 0;          // the set the next K1 deals into
    uint32_t deal_frames = 0, deal_fallbacks = 0;   // diagnostics: forwards whose K1 dealt / of those, the ones whose order had to be queued again (a bucket overflowed)
    uint32_t deal_cap_override = 0;   // != 0: slots per bucket instead of deal_capacity(n) (bh_debug_set_deal_capacity of the test-hooks library only)
    bool knob_dsort_deal = true;      // option dsort_deal: K1 deals the listed splats into the depth sort's buckets (0: histogram + split launches)
    bool knob_dsort_splitters = true; // option dsort_splitters: the split digit from the previous frame's quantiles (0: always the linear split)
    bool adam_lds_raised = false;     // adam_rowreduced_kernel's > 64 KB dynamic-LDS opt-in was made on this ctx's device
    uint32_t update_lds_raised = 0;   // likewise train_update_kernel: one bit per instantiation (optim.hip launch_train_update)
    size_t lds_optin_max = 0;         // the device's opt-in limit of dynamic LDS per block, 0: not asked yet (optim.hip max_dynamic_lds)
    // developer knobs (A/B measurements): bh_set_option
    bool knob_no_lpt = false;         // option no_lpt: backward tiles in index order
    bool knob_bwd_wide_rows = false;  // option bwd_wide_rows: the blend backward forms the accumulator's addresses in 64 bits whatever its size (rasterize.hip)
    bool knob_bwd_jobs = true;        // option bwd_jobs: the blend backward works on checkpointed segments of the tiles' lists (rasterize.hip)
    bool knob_lpt_linear = false;     // option lpt_classes=linear: the work classes of rounds 2-5 (rasterize.hip)
    bool knob_force_exchange = false;       // BH_FORCE_PG: run the gradient-exchange path with a one-rank communicator too (overhead measurement)
    bool knob_break_allreduce = false;      // BH_BREAK_ALLREDUCE: corrupt the library's all-reduce (the bench self-check must notice)
    bool knob_generic_depth_sort = false;   // BH_GENERIC_DEPTH_SORT: the forward's depth order by the generic 32-bit radix sort + scan
    bool knob_zero_grads = false;     // BH_TRAIN_ZERO_GRADS: the single-GPU train step zero-fills its gradient span like the exchange path (A/B)
    uint32_t knob_fail_loss_at = 0;   // BH_TEST_FAIL_LOSS_AT: the k-th bh_train_step on this ctx returns BH_ERR_OOM between its forward and its loss (test hook)
    uint32_t train_steps_seen = 0;
    uint32_t knob_loss_bands = 1;     // BH_LOSS_BANDS=0 (A/B): the fused loss's blocks take their tiles row-major instead of by XCD column bands
    uint32_t knob_tile_sort = 0;      // option tile_sort: 0 auto (bucket sort unless the view's pairs sit in few tiles), 1 bucket, 2 two LSD passes + the offsets kernel
    float auto_exact_share = 0.9f;    // option auto_exact_share: a view whose last cut frame listed more than this share renders complete lists
    bool knob_direct_allreduce = false;   // option grad_allreduce=direct: reduce-scatter + all-gather over grouped send / recv (comm.hip)
    uint32_t knob_k5_exact_spw = 32;  // BH_K5_EXACT_SPW = 16 | 32 | 64 (A/B): splats per wave of K5 for complete lists
    bool knob_no_dormant = false;     // BH_UPDATE_NO_DORMANT (A/B, tests): the update kernel fetches and updates dormant splats like everyone else
    int knob_update_sparse = -1;      // option update_sparse: non-dormant rows up to which an update block takes its one-round-trip path (-1: the default of launch_train_update)
    uint32_t knob_update_rows = 0;    // BH_UPDATE_ROWS: 64 | 128 | 256 splats per block of the update kernel
    uint32_t knob_sort_kpt = 0;       // BH_SORT_KPT: 4 | 8 | 16 keys per thread of the radix sort
    // the update kernel's dormant marks (sign of m2_sh, optim.hip) are trusted only on the state this ctx updated last step
    const void* marks_m2_sh = nullptr; const void* marks_m1_t = nullptr; uint32_t marks_n = 0, marks_step = 0;
    bh::Profiler prof;
};

namespace bh {

int set_error(bh_ctx* ctx, int code, const std::string& msg);
// api.hip: the forward pipeline of one request (arguments already checked), and the host's wait for a tag word a kernel stores
int forward_impl(bh_ctx* ctx, const ForwardRequest& req, BhRenderOut* out);
int wait_host_tag(bh_ctx* ctx, const volatile uint32_t* word, uint32_t want, const char* what);
// api.hip: look up the saved BH_FLAG_BWD_INFO forward or refuse.  `saved` without the flag is refused with `not_bwd_code` (the
// entry points differ: BH_ERR_STATE in api.hip and pose.hip, BH_ERR_INVALID_ARG for the maps) under `who`'s name; then the ctx's
// device is made current and *fs = the saved state of the forward `saved` names — a retained one or the ctx's most recent forward
// (the ctx's own record either way, no copy); anything else is BH_ERR_STATE under `who`'s name (a pending far slice is finished
// first).  Valid until the next call that retains, releases or renders on the ctx.
int find_saved_bwd_forward(bh_ctx* ctx, const BhRenderOut* saved, int not_bwd_code, const char* who, const ForwardState** fs);
// api.hip: the backward kernels on the saved state `fs`.  v_output may be NULL when the call has another term (then K17 does not
// run)
int backward_impl(bh_ctx* ctx, const ForwardState& fs, const float* v_output, const BackwardCall& call);
// api.hip: bh_render_forward and the train step (train.hip): the request's checks, a deferred far-slice decision collected, then forward_impl
int render_forward(bh_ctx* ctx, const ForwardRequest& req, BhRenderOut* out);
// api.hip: what the bh_render_backward*_saved entry points share.  `required`: the cotangents that entry refuses to do without;
// a term of `call` whose cotangent is NULL is an optional one the caller left out.  In this order: the null-argument refusal, the
// distortion-kind, normal-mode and depth-mode refusals, find_saved_bwd_forward(not_bwd_code), the null-transforms refusal (an
// entry that accepts a normal term has it), backward_impl.  Every text carries `who`.  NEED_V_FEATURES: the feature term's four
// pointers join the null-argument refusal, and its channel count is refused behind the depth-mode refusals.
enum : uint32_t { NEED_V_OUTPUT = 1u, NEED_V_DEPTH = 2u, NEED_V_NORMAL = 4u, NEED_V_DISTORTION = 8u, NEED_V_VIEWMAT = 16u, NEED_V_FEATURES = 32u, NEED_V_INTRINSICS = 64u };
int backward_entry(bh_ctx* ctx, const char* who, int not_bwd_code, uint32_t required, const BhRenderOut* saved, const float* v_output, BackwardCall call);
// depth.hip: the depth term between K17 and K18 (raw sums into v_combined; *v_z = the per-splat vector it filled), and a v_z ->
// v_mean behind K18 (the depth term's vector, the distortion term's, or the one both filled)
int launch_depth_backward(bh_ctx* ctx, const ForwardState& fs, const DepthTerm& term, float* v_combined, float** v_z);
// mark_rows (the single-GPU train step's ROW_MARKS span): device_map_blend.h claim_grad_row
int launch_depth_vz_scatter(bh_ctx* ctx, const ForwardState& fs, const float* v_z, float* v_transforms, bool mark_rows, float* v_sh_coeffs,
                            float* v_raw_opacities, float* v_refine_weight);
int launch_depth_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t mode, float* out_depth);
// normal.hip: the normal term between K17 and K18 (raw sums into v_combined; *v_n = the per-splat [Nv,3] vector it filled), and
// Vn -> v_quat behind K18 and depth's scatter; mark_rows as launch_depth_vz_scatter's
int launch_normal_backward(bh_ctx* ctx, const ForwardState& fs, const NormalTerm& term, const float* transforms, float* v_combined, const float** v_n);
int launch_normal_vn_scatter(bh_ctx* ctx, const ForwardState& fs, const float* v_n, const float* transforms, float* v_transforms, bool mark_rows,
                             float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight);
// ... and the normal map `mode` of a saved forward with something listed (bh_render_normal, the train step's normal term)
int launch_normal_map(bh_ctx* ctx, const ForwardState& fs, const float* transforms, uint32_t mode, float* out);
// normal_loss.hip: the fused normal-consistency operator on the ctx stream (arguments already checked; weight > 0).  accum != NULL (train
// step): loss[0] is added to accum[0] in f32 and the total copied to accum_host
int launch_normal_loss(bh_ctx* ctx, const BhCamera& cam, const float* normal, const float* depth, const float* image, uint32_t h, uint32_t w, float weight,
                       bool accumulate_v_depth, float* loss, float* v_normal, float* v_depth, float* accum, float* accum_host);
// distortion.hip: the distortion term between K17 and K18, behind the depth term's replay (raw sums into v_combined).  *v_z in: the
// depth term's filled vector, or NULL without one; out: the vector the ONE scatter behind K18 reads — the same with this term's v_z
// added, or a vector of the term's own
int launch_distortion_backward(bh_ctx* ctx, const ForwardState& fs, const DistortionTerm& term, float* v_combined, float** v_z);
// ... the distortion map (moments: the moment map [H,W,4]) of a saved forward with something listed, the kind's check and the loss
// (accum as launch_depth_loss's)
int launch_distortion_map(bh_ctx* ctx, const ForwardState& fs, const DistortionTerm& term, bool moments, float* out);
int check_distortion_kind(bh_ctx* ctx, uint32_t kind, float near_z, float far_z, const char* who);
int launch_distortion_loss(bh_ctx* ctx, const float* map, uint32_t h, uint32_t w, uint32_t channels, float weight, float* loss, float* accum,
                           float* accum_host);
// features.hip: the feature term between K17 and K18 (raw sums into v_combined; *v_compact = the compact [Nv,C] vector it filled;
// the dense v_features is cleared), and the compact vector -> the rows of v_features behind K18
int launch_feature_backward(bh_ctx* ctx, const ForwardState& fs, const FeatureTerm& term, float* v_combined, const float** v_compact);
int launch_feature_scatter(bh_ctx* ctx, const ForwardState& fs, const FeatureTerm& term, const float* v_compact);
// ... the pieces of a feature map of a saved forward with something listed: features[gid, :] -> the compact rows `feat` [Nv,C], and
// their blend into out [H,W,C]; feature_term_rows: the address of the compact rows a FeatureTerm::compact must have (SLOT_FEATURES,
// sized for the backward); the fused loss (the target is already checked; accum as launch_depth_loss's)
int launch_feature_gather(bh_ctx* ctx, const ForwardState& fs, const float* features, uint32_t channels, float* feat);
int launch_feature_forward(bh_ctx* ctx, const ForwardState& fs, uint32_t channels, const float* feat, float* out);
int feature_term_rows(bh_ctx* ctx, const ForwardState& fs, uint32_t channels, float** feat);
int launch_feature_loss(bh_ctx* ctx, const float* map, const BhFeatureTarget& t, float* loss, float* v_map, float* accum, float* accum_host);
// depth_loss.hip: the fused depth loss on the ctx stream (the target is already checked; weight > 0).  accum != NULL (train step):
// accum[0] += loss[0], and the sum is stored to accum_host too
int launch_depth_loss(bh_ctx* ctx, const float* depth, const BhDepthTarget& t, float* loss, float* v_depth, float* accum, float* accum_host);
// ... what the pixel losses share (depth, normal consistency, distortion): the partial rows of a map of `pixels` pixels
// (SLOT_PIXEL_LOSS; NULL: out of memory) with *blocks = the grid that fills them (DL_WG threads each, at most DL_MAX_BLOCKS), and
// the final block: loss = { f32(c * column 0 of the f64 rows), column 1 }, accum as above
double* loss_partials(bh_ctx* ctx, uint64_t pixels, uint32_t* blocks);
int launch_loss_pair_final(bh_ctx* ctx, uint32_t rows, const double* partials, float c, float* loss, float* accum, float* accum_host);
// project.hip: the pose gradient v_viewmat [12] of the RasterizeGrads rows K18 left in v_combined (brush_hip_pose.h)
int launch_pose_grad(bh_ctx* ctx, const ViewUniforms& u, uint32_t nv, bool mip, uint32_t sh_degree, const float* transforms,
                     const float* sh, const uint32_t* gid, const float* v_combined, float* v_viewmat);
// intrinsics.hip: the intrinsics gradient v_intrinsics [4] of the same rows (brush_hip_intrinsics.h)
int launch_intrinsics_grad(bh_ctx* ctx, const ViewUniforms& u, uint32_t nv, bool mip, const float* transforms, const uint32_t* gid,
                           const float* v_combined, float* v_intrinsics);
// exposure.hip: y = A x + b with the row of `view` (1 .. n_views), and its backward: v_img = A^T v_exposed (in place
// allowed), grad[view] = v_m, and one Adam step of the row when `update` (brush_hip_exposure.h).  The view is already checked.
int launch_exposure_apply(bh_ctx* ctx, const bh_exposure* tab, uint32_t view, const float* img, uint32_t h, uint32_t w, float* out);
int launch_exposure_backward(bh_ctx* ctx, bh_exposure* tab, uint32_t view, const float* img, const float* v_exposed, uint32_t h, uint32_t w,
                             float* v_img, bool update);
// bilagrid.hip: the slice of `img` with the grid of `view` (1 .. n_views), its backward: v_img (in place allowed), grad[view] =
// v_g + tv_weight dTV and one Adam step of the row when `update`, and TV of the row into value[0]; accum as launch_depth_loss's, with
// weight * TV added (brush_hip_bilagrid.h).  The view and the image size are already checked.
int launch_bilagrid_slice(bh_ctx* ctx, const bh_bilagrid* tab, uint32_t view, const float* img, uint32_t h, uint32_t w, float* out);
int launch_bilagrid_backward(bh_ctx* ctx, bh_bilagrid* tab, uint32_t view, const float* img, const float* v_sliced, uint32_t h, uint32_t w, float* v_img,
                             float tv_weight, bool update);
int launch_bilagrid_tv(bh_ctx* ctx, const bh_bilagrid* tab, uint32_t view, float* value, float weight, float* accum, float* accum_host);
float* bilagrid_tv_scratch(bh_ctx* ctx);   // four floats of SLOT_BILAGRID for the train step's TV value
// envmap.hip: out = img over the map seen through `cam`, and its backward: v_img (in place allowed), the map's gradient = v_E and — when
// `update` — one Adam step of the table on gscale * v_E (brush_hip_envmap.h).  Camera and image size are already checked.  A
// non-finite max |v_out|: check_host reads it back and refuses; otherwise the kernels behind the max pass do nothing.  launch_envmap_adam:
// the step alone, on the gradient as it stands (the train step sums it over the ranks first).
int check_envmap_frame(bh_ctx* ctx, const BhCamera* cam, uint32_t h, uint32_t w, const char* who);
int launch_envmap_composite(bh_ctx* ctx, const bh_envmap* map, const BhCamera& cam, const float* img, uint32_t h, uint32_t w, float* out);
int launch_envmap_backward(bh_ctx* ctx, bh_envmap* map, const BhCamera& cam, const float* img, const float* v_out, uint32_t h, uint32_t w, float* v_img,
                           bool update, float gscale, bool check_host);
int launch_envmap_adam(bh_ctx* ctx, bh_envmap* map, float gscale);
// lists.hip — the per-tile cut-list policy (BH_FLAG_SLICED_LISTS, automatic mode) and the far job
// The state of the view a frame of `req` renders (created on first use), or nullptr: a forward-only frame (casual) without a view
// id whose camera is new, or a failed allocation.  A second attempt (!req.allow_cut) leaves the view's gap and LRU stamp alone.
ViewState* frame_view(bh_ctx* ctx, const ForwardRequest& req, uint32_t tile_bw, uint32_t tile_bh, bool casual);
// whether this frame of `vs` lists against its cuts (else complete lists); counts down the view's complete-list frames
bool cut_this_frame(const bh_ctx* ctx, ViewState* vs, bool allow_cut);
// the view's device table: [T] depth cuts | [T] per-tile work of its last frame | [VIEW_SPL_WORDS] depth-sort splitter tables
uint32_t* view_table(const ViewState* vs);
// ... the splitter table a frame uses ([0] complete lists, [1] cut lists), and whether a frame has written it
uint32_t* view_splitters(ViewState* vs, bool cut, bool** written, uint32_t** listed = nullptr);
// margin (in % of a tile's depth rank) the blend kernel of this frame writes behind every tile's last useful splat
uint32_t cut_margin_pct(const bh_ctx* ctx, const ViewState* vs);
// the near slice's pair budget of a BH_FLAG_SLICED_LISTS frame with ni > 0 pairs (== ni: one slice, the complete lists).
// cut_view: the view whose cuts this frame's lists end at (near_total pairs in front of them), or NULL
uint32_t list_budget(bh_ctx* ctx, ViewState* cut_view, uint32_t near_total, uint32_t ni);
// a frame of `vs` with ni pairs has been queued: its blend kernel leaves what every tile needed in the table
void view_rendered(ViewState* vs, uint32_t ni);
int enqueue_far_slice(bh_ctx* ctx, const FarJob& j);
int finish_far_slice(bh_ctx* ctx, bool* launched);
// bh_train_step: the pending job's view has missed at least twice lately — decide before the loss kernels are queued
bool far_job_decides_first(const bh_ctx* ctx);
// bh_train_step failed: forget the pending job (its view's next frame renders complete lists)
void drop_far_job(bh_ctx* ctx);
// after ANY host wait on the ctx stream: hand the last train step's loss (pinned staging word) to its BhTrainStats
inline void deliver_pending_loss(bh_ctx* ctx) {
    if (ctx->pending_loss_dst) {
        *ctx->pending_loss_dst = reinterpret_cast<const volatile float*>(ctx->host_counters)[HOST_LOSS_WORD];
        ctx->pending_loss_dst = nullptr;
    }
}
int check_hip(bh_ctx* ctx, hipError_t e, const char* what);
// lpips.hip: the train step's LPIPS term on the frame's image: *loss += w * LPIPS (and loss_host), v_output.rgb += w * dLPIPS/dimg
int lpips_train_term(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, const float* bg, float* v_output,
                     float* loss, float* loss_host);
// ply.hip: the comment lines every exported PLY header carries (export.rs:188-193), shared by both writers
std::string ply_header_comments(uint32_t sh_degree, bool render_mip, const float* up_axis);
// image.hip: image::imageops::resize.  A pass's weight table is built on the host (resize_table_bytes bytes,
// 16-byte multiple); enqueue_resize runs the vertical pass into tmp (w * nh * channels floats), then the horizontal one into out.
enum ResizeOut : int { RESIZE_OUT_U8 = 0, RESIZE_OUT_PACKED = 1, RESIZE_OUT_PACKED_PREMUL = 2 };
size_t resize_table_bytes(uint32_t src, uint32_t dst, uint32_t filter);
void build_resize_table(uint32_t src, uint32_t dst, uint32_t filter, void* host);
// ... the same table from a process-wide cache (built on a miss; thread-safe)
using ResizeTable = std::shared_ptr<const std::vector<uint8_t>>;
ResizeTable resize_table(uint32_t src, uint32_t dst, uint32_t filter);
hipError_t enqueue_resize(hipStream_t st, const uint8_t* src, uint32_t w, uint32_t h, uint32_t channels, uint32_t nw, uint32_t nh,
                          const int32_t* vtab, const int32_t* htab, float* tmp, void* out, int mode);
// img (RGB8 / RGBA8) + mask [pixels] u8 -> packed rgba8 with alpha = mask (255 - mask), premultiplied or not
hipError_t enqueue_mask_merge(hipStream_t st, const uint8_t* img, uint32_t channels, const uint8_t* mask, uint64_t pixels, int invert,
                              int premultiply, uint32_t* out);
// Grow-only allocation of a scratch slot; returns nullptr (and sets the error) on failure.
void* ensure(bh_ctx* ctx, Slot s, size_t bytes);

struct ProfScope {
    bh_ctx* ctx;
    int idx = -1;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(bh_ctx* c, const char* name, bool dominant = false);
    ~ProfScope();
};

#define BH_HIP(ctx, expr)                                            \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) return bh::check_hip(ctx, _e, #expr);  \
    } while (0)
#define BH_TRY(expr)            \
    do {                        \
        int _rc = (expr);       \
        if (_rc != 0) return _rc; \
    } while (0)
#define BH_LAUNCH_CHECK(ctx, what)                                      \
    do {                                                                \
        hipError_t _e = hipGetLastError();                              \
        if (_e != hipSuccess) return bh::check_hip(ctx, _e, what);      \
    } while (0)

ViewUniforms make_uniforms(const BhCamera& c);

// ---- launchers (each in its own TU) --------------------------------------------
// project.hip

// Buffers K1 clears on the way (every splat thread stores a few zeros: three fill launches fewer per forward).
struct ForwardPrep {
    unsigned long long* next_counters = nullptr;  // the idle half of the counter ping-pong, cleared for the next forward
    uint32_t* visible = nullptr;                  // visible flags (K16 sets them), or NULL
    uint32_t visible_words = 0;
    uint32_t* tile_table = nullptr;               // tile_offsets + the work-class counters behind it
    uint32_t tile_words = 0;
    float4* span = nullptr;                       // train step: the gradient span of the exchange buffer (grid-stride float4 clear)
    uint32_t span_f4 = 0;
    uint32_t* slice_table = nullptr;              // depth-sliced forward: control words + done bits + far tile offsets
    uint32_t slice_words = 0;
    // the forward blend's tile order: blocks 0..7 sort the tiles of XCD band b by the view's last per-tile work (descending)
    const uint32_t* order_work = nullptr;         // [T] (global tile ids), or NULL
    uint32_t* order_out = nullptr;                // [8][ceil(order_tiles/8)] local tile ids, 0xFFFFFFFF behind a short band
    uint32_t order_tiles = 0, order_tile_begin = 0;
    uint32_t order_mode = 1;                      // 1: descending work   2: dealt (consecutive blocks take every 8th rank)
    uint32_t band_mode = 0;                       // context.h XCD BANDS
    uint32_t* split_out = nullptr;                // split_count[8] | split_scratch (SPLIT_TAIL_WORDS), or NULL: no tile is split
    float split_factor = 2.5f;                    // a tile is split when its forecast work >= max(split_min, split_factor * the band's mean)
    uint32_t split_min = SPLIT_MIN_WORK;
    float split_of_max = 0.45f;                   // ... and >= this share of the band's heaviest tile
    bool list_all_visible = false;                // A/B knob BH_CUT_SORT_ALL: per-tile cuts sort and number EVERY visible splat
    DealArgs deal;                                // the listed splats go straight into the depth sort's buckets (depth_deal.h)
    unsigned long long* deal_next = nullptr;      // the idle deal counter set [DEAL_SET_U64], cleared for the next forward
};
int launch_project_forward(bh_ctx* ctx, const ViewUniforms& u, uint32_t n, bool mip, uint32_t sh_degree, const float* transforms,
                           const float* sh, const float* raw_opac, uint32_t* depth_keys, uint32_t* isect_counts, float* max_radius,
                           float* projected_by_gid, uint32_t* counters, const ForwardPrep& prep, uint32_t* zcut = nullptr,
                           uint32_t* near_counts = nullptr);
int launch_project_visible(bh_ctx* ctx, uint32_t nv, const float* projected_by_gid, const uint32_t* gid, float* projected);
// budget: only splats whose slot range ends at or below it are emitted (the near slice of a depth-sliced forward; 0xFFFFFFFF =
// all); slice_info (device, 2 words) then receives the slice's splat count and pair count.
int launch_map_gaussians(bh_ctx* ctx, uint32_t nv, const ViewUniforms& u, const float* projected_by_gid, const uint32_t* gid,
                         float* projected, const uint32_t* cum_tiles_hit, uint32_t* tile_ids, uint32_t* isect_gids,
                         float4* zero_span = nullptr, uint32_t zero_f4 = 0, uint32_t budget = 0xFFFFFFFFu, uint32_t* slice_info = nullptr,
                         const uint32_t* zcut = nullptr, const uint32_t* depth_keys_sorted = nullptr, const uint32_t* nv_dev = nullptr, uint32_t pair_cap = 0xFFFFFFFFu);
int launch_map_gaussians_far(bh_ctx* ctx, uint32_t nv, const ViewUniforms& u, const float* projected_by_gid, const uint32_t* gid,
                             float* projected, const uint32_t* cum_tiles_hit, uint32_t budget, const uint32_t* done_bits, const uint32_t* gate,
                             uint32_t* counts, uint32_t* block_totals, uint32_t* group_totals, uint32_t* slice_info, uint32_t* tile_ids, uint32_t* isect_gids);
int launch_project_backward(bh_ctx* ctx, const ViewUniforms& u, uint32_t nv, bool mip, uint32_t sh_degree,
                            const float* transforms, const float* sh, const float* raw_opac, const uint32_t* gid,
                            float* v_combined, float* v_transforms, float* v_sh, float* v_raw_opac,
                            float* v_refine, bool mark_written = false, const float* projected = nullptr);
// sort.hip
// Group tables of one histogram -> scatter pair (SORT_GROUP_BLOCKS).  The histogram blocks ADD into `sums`, which therefore has to be
// zero, and nothing in front of them on the stream is there to clear it: the ctx keeps two sets, the histogram kernel of every sort
// clears the set the sort BEFORE it used (`stale`, plain stores spread over its grid) and the sets change roles.
struct SortGroups {
    uint32_t* sums = nullptr;    // [words] zero on entry
    uint32_t* stale = nullptr;   // [stale_words] to be cleared by the kernel that adds into `sums`
    uint32_t stale_words = 0;
};
inline uint32_t sort_group_count(uint32_t nblocks) { return (nblocks + SORT_GROUP_BLOCKS - 1u) / SORT_GROUP_BLOCKS; }
// Every call is followed by exactly ONE histogram launch on ctx->stream that takes `out`: that launch clears the stale set, and the
// roles of the two sets have changed when this returns.
int sort_groups_next(bh_ctx* ctx, size_t words, SortGroups* out);
// Up to SORT_DIRECT_GROUPS groups (1024 blocks) a scatter block adds up the group rows in front of it itself.  That is nblocks x
// ngroups KB of table reads, quadratic in the key count: 16 MB at 512 blocks, 360 MB at 2930 (6 M splats: measured, +50 us per step
// over the two sorts).  Longer sorts therefore keep ONE small launch between histogram and scatter (5.6 us): sort_groups_scan turns
// the group table into exclusive prefixes over the groups in place and stores the digit totals, and a scatter block reads one group
// row and the totals whatever the length.  Measured on both sides of the threshold against the row-scan version (EXPERIMENTS.md):
// 2 M splats (977 depth-sort blocks, direct) -1.6 % of the step, 3 M (1465, scanned) -1.1 %, 6 M / 4K (2930, scanned) -0.4 %.
constexpr uint32_t SORT_DIRECT_GROUPS = 32;
inline bool sort_groups_scanned(uint32_t ngroups) { return ngroups > SORT_DIRECT_GROUPS; }
// sums: `tables` tables of [ngroups][256] -> exclusive prefixes over the groups, in place; totals[tables][256] <- the column sums
int sort_groups_scan(bh_ctx* ctx, uint32_t* sums, uint32_t ngroups, uint32_t tables, uint32_t* totals);
// (the device side — a scatter block's offsets, the clearing of the stale set — is sort_groups.h, for sort.hip and depth_sort.hip)
int radix_argsort(bh_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t bits,
                  uint32_t* out_keys, uint32_t* out_vals);
// the same with the number of pairs in device memory (host: only the bound n_max): n = min(*n_dev, n_max), 0 if *gate == 0
// (gate may be NULL); the result is written *out_base elements into out_keys / out_vals (out_base may be NULL).  Not in place.
int radix_argsort_dev(bh_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint32_t n_max, const uint32_t* n_dev, const uint32_t* gate,
                      const uint32_t* out_base, uint32_t bits, uint32_t* out_keys, uint32_t* out_vals, uint32_t alloc_n = 0);
// sort.hip — the forward's tile sort AND its offsets table in four launches (high digit first, parts of 4096 pairs finish);
// bits in 9..16 and n <= 16 M (tile_sort_supported), the table zero on entry
bool tile_sort_supported(uint32_t bits, uint32_t n);
int tile_sort_offsets(bh_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t bits, uint32_t num_tiles,
                      uint32_t* out_keys, uint32_t* out_vals, uint32_t* tile_offsets, uint32_t alloc_n = 0);
// depth_sort.hip — the forward's depth ordering: stable argsort of the depth keys + inclusive scan of the tile counts in that
// order, three launches.  minmax: the second part of a counter set (K1).  cum == NULL: no scan.  rb_*: the first launch also adds
// up counter set rb_set into the pinned host words rb_host (HOST_SUM_WORDS) and rb_done is recorded behind it.
bool depth_sort_supported(uint32_t n);
int depth_sort_scan(bh_ctx* ctx, const uint32_t* keys, const uint32_t* minmax, const uint32_t* counts, uint32_t n, uint32_t* out_keys,
                    uint32_t* out_vals, uint32_t* cum, const uint32_t* rb_set = nullptr, uint32_t* rb_host = nullptr, hipEvent_t rb_done = nullptr,
                    uint32_t rb_tag = 0, uint32_t* rb_dev = nullptr, uint32_t* spl = nullptr, bool* spl_written = nullptr, const DealArgs* dealt = nullptr);
// ... or ONE launch, when K1 dealt the listed splats into the buckets itself (depth_deal.h): decided before K1 is queued
int depth_deal_prepare(bh_ctx* ctx, uint32_t n, const uint32_t* spl, bool table_usable, ForwardPrep* prep);
bool depth_deal_table_usable(uint32_t listed_by_writer);
// scan.hip — inclusive scan; if `gather` != nullptr the input is in[gather[i]]. exclusive: out[i] = sum_{j<i}.
// gate != NULL: a device word; 0 there turns the launches into no-ops (the depth-sliced forward's second slice)
int prefix_sum(bh_ctx* ctx, const uint32_t* in, const uint32_t* gather, uint32_t n, uint32_t* out, bool exclusive, const uint32_t* gate = nullptr);
// rasterize.hip
int launch_tile_offsets(bh_ctx* ctx, const uint32_t* tile_ids_sorted, uint32_t num_isect, uint32_t num_tiles,
                        uint32_t* tile_offsets, bool pre_zeroed = false);
// the list's length in device memory (min(*n_dev, n_max), 0 if *gate == 0); it starts *base entries into tile_ids_sorted and the
// offsets written are absolute (gate / base may be NULL).  The table must already be zero.
int launch_tile_offsets_dev(bh_ctx* ctx, const uint32_t* tile_ids_sorted, uint32_t n_max, const uint32_t* n_dev, const uint32_t* gate,
                            const uint32_t* base, uint32_t num_tiles, uint32_t* tile_offsets);

// lpt: the longest-first tile order scratch (8*16 counters directly behind tile_offsets, then the class lists); NULL = index order
int launch_rasterize(bh_ctx* ctx, const ViewUniforms& u, const float bg[3], bool bwd_info, bool smooth,
                     const uint32_t* isect_gids, uint32_t* tile_offsets, const float* projected,
                     const uint32_t* global_from_compact, float* out_img, uint32_t* out_packed, float* visible,
                     uint32_t* lpt, float class_width, int phase = 0, const RasterSlice* slice = nullptr);
int launch_rasterize_backward(bh_ctx* ctx, const ViewUniforms& u, const float bg[3], bool smooth,
                              const uint32_t* isect_gids, const uint32_t* tile_offsets, const float* projected,
                              const float* out_img, const float* v_output, float* v_combined, const uint32_t* lpt,
                              const uint32_t* tile_offsets_far = nullptr, bool want_refine = true, const BwdJobs* jobs = nullptr,
                              uint32_t accum_rows = 0u);   // rows of v_combined (0: not known)
// loss.hip
int launch_image_loss_forward(bh_ctx* ctx, const float* pred, const uint32_t* gt, uint32_t channels, uint32_t h,
                              uint32_t w, const BhLossConfig& cfg, float* loss_map);
int launch_image_loss_backward(bh_ctx* ctx, const float* pred, const uint32_t* gt, const float* dl_dmap,
                               float dl_const, uint32_t channels, uint32_t h, uint32_t w, const BhLossConfig& cfg,
                               float* dl_dpred);
// loss_fused.hip
int launch_image_loss_fused(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt, uint32_t h, uint32_t w, const BhLossConfig& cfg,
                            bool alpha_match, float dl_rgb, float dl_alpha, float* loss_out, float* v_output, float* loss_host = nullptr,
                            uint32_t* started_host = nullptr, uint32_t started_tag = 0);
int launch_image_loss_fused_window(bh_ctx* ctx, const float* img_hwc4, const uint32_t* gt, uint32_t h, uint32_t w, const BhLossConfig& cfg,
                                   bool alpha_match, float dl_rgb, float dl_alpha, uint32_t tile_y0, uint32_t tile_y1, float* loss_out,
                                   float* v_output, float* loss_host = nullptr, uint32_t* started_host = nullptr, uint32_t started_tag = 0);
// optim.hip
int launch_adam(bh_ctx* ctx, float* param, const float* grad, float* m1, float* m2, uint64_t rows, uint32_t row_len,
                const float* col_scale, float lr, uint32_t t, bool reduce_m2, float beta1, float beta2, float eps, float gscale = 1.0f);
// (gscale: a factor on every gradient, full second moment only — the feature field's update under data parallelism)
// statistics + the three Adam updates of a train step in one launch (tab_t: per-column lr of `transforms`)
// noise != NULL: the visibility-gated mean noise of train.rs:389-416, drawn on the device (device_rng.h), rides on the same launch
struct NoiseArgs { uint64_t seed; uint32_t step; float scale, clamp_abs; };
struct UpdateCall {
    const float *g_transforms, *g_sh, *g_opac;               // gradients [n,10], [n,3C], [n]
    const float *refine_weight, *visible, *screen_radius;   // the frame's per-splat outputs the statistics gather
    float gscale;            // factor on every gradient (1/world for data parallel over cameras, else 1)
    bool vis_clamp;          // `visible` arrives summed over strips: min(v, 1)
    float tab_t[10];         // lr_mean x3, lr_rotation x4, lr_scale x3
    float lr_sh, sh_rest_scale, lr_opac;   // SH: DC at lr_sh, bands >= 1 at lr_sh * sh_rest_scale
    uint32_t t;              // 1-based step
    float beta1, beta2, eps;
    const NoiseArgs* noise;  // NULL: no noise on this launch
    bool masked_rows;        // the gradient tensors were not zero-filled: row i counts iff the sign bit of refine_weight[i] is set
};
int launch_train_update(bh_ctx* ctx, const BhTrainState* st, const UpdateCall& c);
int launch_gather_stats(bh_ctx* ctx, float* refine_weight_norm, float* vis_weight, float* max_screen_size,
                        const float* refine_weight, const float* visible, const float* screen_radius, uint64_t n);
// samples == NULL: drawn on the device from (seed, step, splat)
int launch_mean_noise(bh_ctx* ctx, float* transforms, const float* raw_opac, const float* visible,
                      const float* samples, uint64_t n, float noise_scale, float clamp_abs, uint64_t seed = 0, uint32_t step = 0);
int launch_normal_samples(bh_ctx* ctx, float* out, uint64_t n, uint64_t seed, uint32_t step);

// filter3d.hip — Mip-Splatting 3D filter (scale floor): fold, its VJP, the floor itself
int launch_fold_min_scale(bh_ctx* ctx, const float* transforms, const float* raw_opac, const float* min_scale, uint32_t n,
                          float* out_transforms, float* out_raw_opac);
int launch_fold_min_scale_backward(bh_ctx* ctx, const float* transforms, const float* raw_opac, const float* min_scale, uint32_t n,
                                   float* v_transforms, float* v_raw_opac);
int launch_compute_min_scale(bh_ctx* ctx, const float* transforms, uint32_t n, const float* view_cams, uint32_t k, float factor, float* out);

// comm.hip — in-place all-reduce of `count` floats over the ctx's RCCL communicator, on the ctx stream
int comm_allreduce(bh_ctx* ctx, float* buf, uint64_t count, bool max_op);   // on ctx->stream
int comm_exchange_strip_halos(bh_ctx* ctx, float* img, uint32_t h, uint32_t w, uint32_t row_begin_px, uint32_t row_end_px);

// exchange.hip — compaction kernels of the mask-keyed gradient exchange
int launch_union_index(bh_ctx* ctx, const float* visible_sum, uint32_t n, uint32_t* block_scratch /*[n/4096+2]*/, uint32_t* count_dev,
                       uint32_t* idx);
int launch_exchange_rows(bh_ctx* ctx, bool gather, const uint32_t* idx, uint32_t count, uint32_t c3, float* g_tr, float* g_sh, float* g_op,
                         float* g_ref /*NULL = no refine-weight column*/, float* compact);

}  // namespace bh
