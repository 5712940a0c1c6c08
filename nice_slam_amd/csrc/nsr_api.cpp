// nsr_api.cpp -- the C ABI of libnsr.so (see include/nsr.h).  Compiled as HIP for gfx950.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "nsr_rt.h"
#include "nsr_kernels.h"
// (spelled from two levels up: the library build finds it beside this file, the CPU emulator build -- which compiles a copy of
//  this file elsewhere -- through its include path tests/emu)
#include "../../nice_slam_amd/csrc/nsr_recon.h"
#include "../../nice_slam_amd/csrc/nsr_meshdist.h"
#include "../../nice_slam_amd/csrc/nsr_bound.h"
#include "../../nice_slam_amd/csrc/nsr_raster.h"
#include "../../nice_slam_amd/csrc/nsr_view.h"
#include "../../nice_slam_amd/csrc/nsr_imgmetrics.h"
#include "../../nice_slam_amd/csrc/nsr_figure.h"
#include "../../nice_slam_amd/csrc/nsr_frame.h"
#include "../../nice_slam_amd/csrc/nsr_pose.h"
#include "../../nice_slam_amd/csrc/nsr_trajeval.h"
#include "../../nice_slam_amd/csrc/nsr_jpeg.h"
#include "../../nice_slam_amd/csrc/nsr_jpegdec.h"
#include "../../nice_slam_amd/csrc/nsr_png.h"

namespace {

thread_local std::string g_err;

int fail(const std::string &msg) {
    g_err = msg;
    return 1;
}

constexpr int kMaxTiles = 12;            // 12 waves = 768 threads per block
constexpr int kDefaultBwdBlocks = 256;   // persistent-grid cap of the backward kernels: one block per CU (LDS-bound)
constexpr int kLdsLimit = 160 * 1024;
constexpr int kKeyframeBlocks = 256;        // keyframe selection: one block per CU, grid-stride over the keyframes

// ---- launch policy: one value per choice, each the measured winner (profiles/) ----------------------------------
// The three NSR_TEST_* hooks let the CPU emulator tests build variants that reach other shapes of the same code
// (tests/test_emu_parity.py); the library build never defines them.
#ifndef NSR_TEST_FWD_SMALL
#define NSR_TEST_FWD_SMALL 1
#endif
#ifndef NSR_TEST_HOT_CELLS
#define NSR_TEST_HOT_CELLS 6
#endif
#ifndef NSR_TEST_HOT_SLOTS
#define NSR_TEST_HOT_SLOTS 512
#endif
// Small batches (the tracker's 200 rays): a one-launch forward block runs its decoders one after the other, so with few blocks
// the launch takes one block's serial chain while most CUs idle.  Fewer rays per block -> one block per CU as long as the batch
// allows (off: always full 12-tile blocks).
constexpr bool kFwdSmallBlocks = NSR_TEST_FWD_SMALL != 0;
// hot-voxel table of a dX block: samples within kHotCells cells of their ray's origin (0: no table), as many slots as the
// block's LDS has left, at most kHotSlotCap (round 5: 64 slots / 2 cells -> what fits / 6 cells, measured)
constexpr int kHotCells = NSR_TEST_HOT_CELLS;
constexpr int kHotSlotCap = NSR_TEST_HOT_SLOTS;
// dX block deal over the decoder passes by a tile's cost: a pass that owes neither parameter nor ray gradients skips its
// embedding backward (96 of 240 MFMAs, 24 cosines per lane) -- with equal shares the other passes' blocks set the kernel's length
// (`--stepped-grads-only`: dX<3> 95 us against 85 with every decoder's gradients); measured 10 / 8 / 7 / 6 / 5 to 10 for a full
// pass: 92.4 / 85.3 / 82.6 / 79.5 / 80.9 us
constexpr int kDxFullWeight = 10, kDxLightWeight = 6;
// dW block deal: the fine decoder's share (the others: 224): its 288 MFMAs per tile against 224 overstate it -- a tile's time has
// a part that does not scale with the MFMA count (flags, operand reads, sines).  Measured (round 6, log item 22): colour stage
// 240, fine stage 260.
constexpr int kDwWeight = 224;
inline int dw_fine_weight(int stage) { return stage == NSR_STAGE_COLOR ? 240 : 260; }
// finalize: 512 threads = four resident blocks per CU instead of two was measured: 17.4 vs 15.1 us -- the kernel is a chain of
// round trips, not a queue of blocks
constexpr int kFinThreads = 1024;
// three-launch forward: blocks per decoder pass in proportion to the measured cost of a tile (the fine decoder: 288 MFMAs and two
// feature gathers against 240 and one), one block per CU over all passes; waves per block from the largest tile share, at most
// nsr::kDxMaxWaves.  Swept again in round 6: fine stage 12, colour stage 14 against 10 for the others.
constexpr int kFwdWeight = 10;
inline int fwd_fine_weight(int stage) { return stage == NSR_STAGE_FINE ? 12 : 14; }

inline unsigned nblk(long long n, int tb) { return (unsigned)((n + tb - 1) / tb); }

// ---- caller-allocated workspaces ---------------------------------------------------------------------------------------------
inline long long pad16(long long bytes) { return (bytes + 15) & ~15ll; }

// a workspace is described ONCE, by a function that takes its pieces from a Carve in order: without a base it measures (the
// size entry returns `at`), with the caller's pointer it binds (the working entries)
struct Carve {
    char *base;
    long long at = 0;
    explicit Carve(const void *workspace = nullptr) : base(static_cast<char *>(const_cast<void *>(workspace))) {}
    // `count` elements; the next piece starts 16-byte aligned
    template <typename T> T *take(long long count) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += pad16(count * (long long)sizeof(T));
        return p;
    }
};
// the bytes of the workspace that `describe` lays out for P, bound to P where the caller's workspace is given
template <typename Params>
long long carve(void (*describe)(Params &, Carve &), Params &P, const void *workspace = nullptr) {
    Carve c(workspace);
    describe(P, c);
    return c.at;
}

int finish(const char *what) {
    if (const char *e = nsr::rt_check_last()) return fail(std::string(what) + ": " + e);
    return 0;
}

// ---- a render stage: its decoder slots and passes -----------------------------------------------------------------------------
// The coarse stage runs the coarse decoder alone; the middle, fine and colour stages run the decoders from the middle one up to
// their own (middle 1, fine 2, colour 3), one decoder pass each: pass p is slot first + p.  A block of the pass, dX and dW kernels
// serves ONE pass -- that decoder's operand stream sits in its LDS.
struct StageSlots {
    int first, last, passes;
    explicit StageSlots(int stage)
        : first(stage == NSR_STAGE_COARSE ? NSR_COARSE : NSR_MIDDLE), last(stage == NSR_STAGE_COARSE ? NSR_COARSE : stage), passes(last - first + 1) {}
    int slot(int pass) const { return first + pass; }
    int pass_of(int slot) const { return slot - first; }
    // the largest f(slot) over the stage's slots
    template <typename F> int most(F f) const { int m = 0; for (int s = first; s <= last; ++s) m = std::max(m, (int)f(s)); return m; }
};
// floats between two partial images of the gradient blob: the coarse decoder's count, else the fine decoder's (the largest)
int partial_stride(int stage) { return nsr::param_total(stage == NSR_STAGE_COARSE ? NSR_COARSE : NSR_FINE); }

inline long long tiles_of(long long n_points) { return (n_points + nsr::kTile - 1) / nsr::kTile; }

// ---- the block deal -------------------------------------------------------------------------------------------------------------
// `total` blocks over the decoder passes in proportion to a weight: blocks [beg[p], beg[p + 1]) serve pass p.  A share is
// floor(total * w / sum of w) -- or, for the last pass with `remainder_to_last`, what the others left --, raised to 1, clamped
// to `tiles`; 0 where w == 0 or p >= passes.  (Raised shares can push the sum past `total`: the callers that size a workspace by
// `total` check beg[3], see deal_bwd.)
void deal_blocks(int beg[4], int total, const int wgt[3], int passes, long long tiles, bool remainder_to_last) {
    int wsum = 0, used = 0;
    for (int p = 0; p < passes; ++p) wsum += wgt[p];
    beg[0] = 0;
    for (int p = 0; p < 3; ++p) {
        long long n = 0;
        if (p < passes && wgt[p] > 0) {
            n = remainder_to_last && p == passes - 1 ? total - used : (long long)total * wgt[p] / wsum;
            if (n < 1) n = 1;
            if (n > tiles) n = tiles;
        }
        used += (int)n;
        beg[p + 1] = beg[p] + (int)n;
    }
}

// ---- launches -----------------------------------------------------------------------------------------------------------------
// raise the dynamic-LDS limit of a kernel once per (kernel, device, size): not a stream operation, but kept out of the
// steady state so that a captured hipGraph contains kernel launches only.  Keyed by the kernel's ADDRESS (all render
// kernels share one function-pointer type) and the current device.
template <typename K>
int launch_cfg(K kernel, int lds_bytes, const char *what) {
    if (lds_bytes > kLdsLimit) return fail(std::string(what) + ": LDS budget exceeded");
    if (lds_bytes <= 48 * 1024) return 0;
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, int> granted;
    const std::pair<const void *, int> key(reinterpret_cast<const void *>(kernel), nsr::rt_current_device());
    std::lock_guard<std::mutex> lock(mu);
    int &g = granted[key];
    if (lds_bytes > g) {
        if (const char *e = nsr::rt_allow_lds(kernel, lds_bytes)) return fail(std::string(what) + ": " + e);
        g = lds_bytes;
    }
    return 0;
}
// a kernel with dynamic LDS: the grant, then the launch
template <typename Params>
int launch_kernel(void (*kernel)(Params), dim3 grid, dim3 block, int lds_bytes, const char *what, void *stream, const Params &P) {
    if (int rc = launch_cfg(kernel, lds_bytes, what)) return rc;
    NSR_LAUNCH(kernel, grid, block, lds_bytes, stream, P);
    return 0;
}
// the run-time stage (or decoder slot) as a compile-time constant: f(Int<stage>()), ST() inside f
template <int N> using Int = std::integral_constant<int, N>;
template <typename F> int with_stage(int stage, F f) {
    return stage == 0 ? f(Int<0>()) : stage == 1 ? f(Int<1>()) : stage == 2 ? f(Int<2>()) : f(Int<3>());
}

// ---- LDS bytes of a block -----------------------------------------------------------------------------------------------------
// the largest need over the stage's decoders.  One-launch forward and eval_points: three aux tables, the block's own bytes, the
// operand stream; pass kernels: aux table, stream, tile counter; dX: aux table, transposed stream, a staging area per wave, tile
// counter (the hot-voxel table and the coarse grid: launch_dx)
int fwd_lds_bytes(int stage, int own_bytes) { return (int)pad16(3 * nsr::AUX_FLOATS * 4) + own_bytes + StageSlots(stage).most(nsr::packed_total) * 4; }
int pass_lds_bytes(int stage) { return (nsr::AUX_FLOATS + StageSlots(stage).most(nsr::packed_total) + 4) * 4; }
int dx_lds_bytes(int stage, int waves) { return (nsr::AUX_FLOATS + StageSlots(stage).most(nsr::packedT_total) + waves * nsr::kDxStg + 4) * 4; }
int dw_lds_bytes(int stage) { return StageSlots(stage).most(nsr::dw_lds_bytes); }

// ---- nsr_render_args.acts ------------------------------------------------------------------------------------------------------
// [passes][tiles][kActSlots][16][16] saved by the forward | [passes][tiles][kDySlots][16][16] dY (dX kernel -> dW kernel) |
// [npad][4] d raw | [npad][4] fp32 positions | [npad][4] doubles: position + depth.  npad = 16 * tiles = the sample points rounded
// up to whole 16-point tiles (DMA pieces of 1 KB): every piece is a multiple of 256 bytes.  Reads P.stage, P.n_rays, P.S.
void describe_acts(nsr::RenderParams &P, Carve &c) {
    const long long passes = StageSlots(P.stage).passes;
    P.act_tiles = tiles_of(P.n_rays * P.S);
    const long long npad = P.act_tiles * nsr::kTile, slot = npad * 16;      // slot: floats between two slots
    c.take<float>(passes * nsr::kActSlots * slot);                           // (= P.acts itself)
    P.dy = c.take<float>(passes * nsr::kDySlots * slot);
    P.draw = c.take<float>(npad * 4);
    P.pf = c.take<float>(npad * 4);
    P.pd = c.take<double>(npad * 4);
}
// the pieces behind the saved activations (null without a buffer) and P.act_tiles; dY is the backward's alone
void bind_acts(nsr::RenderParams &P, const float *acts, bool bwd) {
    carve(describe_acts, P, acts);
    if (!bwd) P.dy = nullptr;
}

// ---- split backward over saved activations (nsr_bwd2.h) -----------------------------------------------------------------
// launch geometry: the dX kernel runs `nb` blocks of `waves` waves per decoder pass (one block per CU over all passes,
// fewer waves per block when the batch is small: every CU gets work); the dW kernel `nimg` blocks per pass, each of which
// leaves one partial image of the gradient blob.
struct SplitGeo { int nb, waves, nimg; };             // dX: blocks per pass, waves per block; dW: images per pass
SplitGeo split_geo(int stage, long long n_rays, int S, int max_blocks) {
    const long long tiles = tiles_of(n_rays * S), per_pass = std::max(1, (max_blocks > 0 ? max_blocks : kDefaultBwdBlocks) / StageSlots(stage).passes);
    SplitGeo G;
    G.waves = (int)std::clamp<long long>((tiles + per_pass - 1) / per_pass, 1, nsr::kDxMaxWaves);
    G.nb = (int)std::clamp<long long>((tiles + G.waves - 1) / G.waves, 1, per_pass);
    G.nimg = (int)std::clamp<long long>(tiles, 1, per_pass);
    return G;
}
// nsr_bwd_args.workspace (floats): [passes][nimg] partial images of the dW kernel, partial_stride floats each | [passes][nb][kDbPart]
// d _B partials of the dX kernel.  (Not a Carve: an image is no multiple of 16 bytes.)
struct BwdWorkspace { long long dbpart, floats; };     // where the d _B partials start, the whole
BwdWorkspace bwd_workspace(int stage, const SplitGeo &G) {
    const long long passes = StageSlots(stage).passes, dbpart = passes * G.nimg * partial_stride(stage);
    return {dbpart, dbpart + passes * G.nb * nsr::kDbPart};
}

// validate + translate the public argument block
int build_params(const nsr_render_args *a, nsr::RenderParams &P, bool need_rays, bool bwd = false) {
    if (!a) return fail("nsr: null argument block");
    if (a->stage < 0 || a->stage > 3) return fail("nsr: stage out of range");
    std::memset(&P, 0, sizeof(P));
    P.stage = a->stage;
    P.n_samples = a->n_samples;
    const bool guided = a->gt_depth != nullptr && a->stage != NSR_STAGE_COARSE;
    P.n_surface = guided ? a->n_surface : 0;
    P.S = P.n_samples + P.n_surface;
    if (P.n_samples < 1 || P.n_surface < 0 || P.S > NSR_MAX_SAMPLES)
        return fail("nsr: n_samples + n_surface must be in [1, 64]");
    if (guided && !a->gt_max) return fail("nsr: gt_max is required when gt_depth is given");
    P.n_rays = a->n_rays;
    if (need_rays) {
        if (a->n_rays < 0) return fail("nsr: negative ray count");
        if (a->n_rays > 0 && (!a->rays_o || !a->rays_d)) return fail("nsr: null ray pointers");
    }
    P.s_magic = P.S > 1 ? (unsigned)(((1ull << 32) + (unsigned)P.S - 1) / (unsigned)P.S) : 0u;     // (S = 1: nsr_kernels.h::ray_of_point)
    // blocks of render_fwd_kernel (its plan, passed on by every entry): up to 12 tiles (768 threads, 3 waves/SIMD, <=168 VGPRs), for
    // small batches fewer (launch policy above)
    const long long want = !bwd && kFwdSmallBlocks ? (P.n_rays + kDefaultBwdBlocks - 1) / kDefaultBwdBlocks : kMaxTiles * nsr::kTile;
    P.rays_per_block = (int)std::max(1ll, std::min<long long>(want, (kMaxTiles * nsr::kTile) / P.S));
    P.tiles_per_block = (P.rays_per_block * P.S + nsr::kTile - 1) / nsr::kTile;
    P.n_groups = (P.n_rays + P.rays_per_block - 1) / P.rays_per_block;
    P.rays_o = a->rays_o;
    P.rays_d = a->rays_d;
    P.acts = a->acts;
    P.acts_masks_only = a->acts_masks_only & 15;
    // activation buffer of the three-launch forward (nsr_fwd2.h): it leaves the sample positions (and, with the fused loss,
    // d raw) for the split backward and keeps its per-sample scratch there
    bind_acts(P, bwd || (a->zvals && a->raw) ? a->acts : nullptr, bwd);
    P.n_points_total = (long long)P.n_rays * P.S;
    P.gt_depth = guided ? a->gt_depth : nullptr;
    P.gt_max = a->gt_max;
    for (int i = 0; i < 3; ++i) { P.blo[i] = a->bound_lo[i]; P.bhi[i] = a->bound_hi[i]; }
    std::memcpy(P.t_uniform, a->t_uniform, sizeof(P.t_uniform));
    std::memcpy(P.t_surface, a->t_surface, sizeof(P.t_surface));
    const StageSlots st(a->stage);
    for (int s = st.first; s <= st.last; ++s) {
        const nsr_grid &g = a->grid[s];
        if (!g.feat) return fail("nsr: missing feature grid for this stage");
        if (g.Z < 1 || g.Y < 1 || g.X < 1) return fail("nsr: bad grid shape");
        if ((long long)g.Z * g.Y * g.X >= (1ll << 25)) return fail("nsr: grid too large for 32-bit byte offsets (2^25 voxels = 4 GB)");
        nsr::GridDev &G = P.grid[s];
        G.feat = g.feat; G.dfeat = g.dfeat; G.gmask = a->grad_voxel_mask[s]; G.Z = g.Z; G.Y = g.Y; G.X = g.X;
        for (int i = 0; i < 3; ++i) {
            if (!(g.hi[i] > g.lo[i])) return fail("nsr: empty normalisation box");
            G.lo[i] = g.lo[i];
            G.ext[i] = g.hi[i] - g.lo[i];
            G.inv[i] = 1.0 / (g.hi[i] - g.lo[i]);
        }
        const nsr_decoder &d = a->dec[s];
        if (!d.params || !d.packed) return fail("nsr: missing decoder parameters / packed stream for this stage");
        P.dec[s].params = d.params; P.dec[s].packed = d.packed; P.dec[s].dparams = d.dparams;
    }
    P.depth = a->depth; P.var = a->var; P.rgb = a->rgb; P.raw = a->raw; P.zvals = a->zvals;
    P.gt_color = a->gt_color; P.keep = a->keep; P.loss = a->loss; P.w_color = a->w_color;
    P.skip_masked = (a->skip_masked && a->keep && a->acts && a->zvals && a->raw) ? 1 : 0;      // (the one-launch forward renders every ray)
    P.dl_depth = a->dl_depth; P.dl_rgb = a->dl_rgb; P.loss_depth = a->gt_depth;
    return 0;
}

// the block ranges of the dX and dW launches, dealt over the decoder passes by a tile's cost (launch policy above)
int deal_bwd(const nsr::RenderParams &P, const SplitGeo &G, int dx_beg[4], int dw_beg[4]) {
    const StageSlots st(P.stage);
    const bool rays = P.d_rays_o != nullptr;
    int dx_wgt[3] = {0, 0, 0}, dw_wgt[3] = {0, 0, 0};
    for (int p = 0; p < st.passes; ++p) {
        const int s = st.slot(p);
        dx_wgt[p] = (P.dec[s].dparams || rays || P.stage == NSR_STAGE_COARSE) ? kDxFullWeight : kDxLightWeight;
        dw_wgt[p] = P.dec[s].dparams ? (s == NSR_FINE ? dw_fine_weight(P.stage) : kDwWeight) : 0;
    }
    // dX: passes * nb blocks; dW: passes * nimg blocks (= partial images) over the decoders that want parameter gradients
    deal_blocks(dx_beg, st.passes * G.nb, dx_wgt, st.passes, P.act_tiles, true);
    deal_blocks(dw_beg, st.passes * G.nimg, dw_wgt, st.passes, P.act_tiles, false);
    // The workspace holds passes * nb d _B partials and passes * nimg partial images.  With the present weights this never fires
    // (tests/test_render_launch_plan.py holds every recorded backward to it): floored shares sum to at most total, one is raised to
    // 1 only where its floor is 0, total >= passes, and the dX shares before the last stay below total (each <= 10 / 16 of it with
    // two passes, 10 / 22 with three).
    if (dx_beg[3] > st.passes * G.nb || dw_beg[3] > st.passes * G.nimg)
        return fail("nsr_render_bwd: the block deal exceeds the workspace (launch-policy weights)");
    return 0;
}

// checks, and the workspace
int bind_bwd(const nsr_bwd_args *b, nsr::RenderParams &P, const SplitGeo &G, bool any_params) {
    if (P.act_tiles * nsr::kTile * 16 * 4 >= (1ll << 31)) return fail("nsr_render_bwd: more than 2^25 sample points in one call (split the ray batch)");
    const StageSlots st(P.stage);
    for (int s = st.first; s <= st.last; ++s)
        if (P.dec[s].dparams && (P.acts_masks_only & (1 | (2 << st.pass_of(s)))))
            return fail("nsr_render_bwd: the forward saved relu masks only for a decoder whose parameter gradients are asked for (acts_masks_only); they need the full activations");
    // (the fine decoder's input is [c_fine | c_mid], decoder.py:182-187: its dW reads the middle pass's saved features)
    if (P.dec[NSR_FINE].dparams && (P.acts_masks_only & (1 | 2)))
        return fail("nsr_render_bwd: the forward saved relu masks only for the middle decoder (acts_masks_only), whose features the fine decoder's parameter gradients read");
    if (any_params) {
        const BwdWorkspace W = bwd_workspace(P.stage, G);
        if (!b->workspace || b->workspace_floats < W.floats) return fail("nsr_render_bwd: workspace too small");
        P.partials = b->workspace;
        P.dbpart = b->workspace + W.dbpart;
    }
    return 0;
}

// the forward's loss epilogue already wrote d raw (for an incoming gradient of 1): used when the caller SAYS that it hands
// back exactly the derivative arrays that forward produced, unmodified (nsr_bwd_args.loss_grads_from_forward); else the
// compositor backward runs here on d_depth / d_var / d_rgb as given
void launch_comp_bwd(const nsr_render_args *a, const nsr_bwd_args *b, nsr::RenderParams &P, void *stream) {
    const bool draw_ready = b->loss_grads_from_forward && a->loss && a->dl_depth && b->d_depth == a->dl_depth && !b->d_var &&
                            (b->d_rgb == nullptr || b->d_rgb == a->dl_rgb) && (P.stage != NSR_STAGE_COLOR || b->d_rgb == a->dl_rgb || !a->gt_color);
    P.draw_scaled = draw_ready ? 0 : 1;
    if (draw_ready) return;
    const int tb = 256, rays_per_block = tb / 64;
    NSR_LAUNCH(nsr::comp_bwd_kernel, dim3(nblk(P.n_rays, rays_per_block)), dim3(tb), 0, stream, P);
}

int launch_dx(nsr::RenderParams &P, const SplitGeo &G, const int dx_beg[4], void *stream) {
    int lds = dx_lds_bytes(P.stage, G.waves);
    // hot-voxel table of a dX block (launch policy above)
    P.hot_slots = 0;
    if (P.stage != NSR_STAGE_COARSE) {
        int slots = (kLdsLimit - lds) / (nsr::kHotRow * 4);
        slots = slots > kHotSlotCap ? kHotSlotCap : slots;
        P.hot_slots = slots < 16 ? 16 : slots;
        lds += P.hot_slots * nsr::kHotRow * 4;
    }
    for (int s = 0; s < 4; ++s) {
        P.hot_z[s] = 0.f;
        if (s == NSR_COARSE || kHotCells <= 0 || !P.grid[s].dfeat) continue;
        double cell = 0.0;
        const int nn[3] = {P.grid[s].X, P.grid[s].Y, P.grid[s].Z};
        for (int ax = 0; ax < 3; ++ax) { const double c = nn[ax] > 1 ? P.grid[s].ext[ax] / (nn[ax] - 1) : 0.0; cell = c > cell ? c : cell; }
        P.hot_z[s] = (float)(kHotCells * cell);
    }
    P.lds_grid_floats = 0;
    if (P.stage == NSR_STAGE_COARSE && P.grid[NSR_COARSE].dfeat) {       // a coarse gradient grid that fits next to the rest
        const long long gf = (long long)P.grid[NSR_COARSE].X * P.grid[NSR_COARSE].Y * P.grid[NSR_COARSE].Z * nsr::kC;
        if (lds + gf * 4 <= kLdsLimit) { P.lds_grid_floats = (int)gf; lds += (int)gf * 4; }
    }
    std::memcpy(P.dx_beg, dx_beg, sizeof(P.dx_beg));
    return with_stage(P.stage, [&](auto ST) {
        const auto kernel = P.d_rays_o ? nsr::render_bwd_dx_kernel<ST(), true> : nsr::render_bwd_dx_kernel<ST(), false>;
        return launch_kernel(kernel, dim3(P.dx_beg[3]), dim3(64 * G.waves), lds, "nsr_render_bwd(dx)", stream, P);
    });
}

int launch_dw(nsr::RenderParams &P, const int dw_beg[4], void *stream) {
    std::memcpy(P.dw_beg, dw_beg, sizeof(P.dw_beg));
    return with_stage(P.stage, [&](auto ST) {
        return launch_kernel(nsr::render_bwd_dw_kernel<ST()>, dim3(P.dw_beg[3]), dim3(64 * nsr::kDwWaves), dw_lds_bytes(P.stage), "nsr_render_bwd(dw)", stream, P);
    });
}

// dparams (+)= the partial images of its dW blocks and the d _B partials of its dX blocks: one job per decoder with gradients
void launch_finalize(const nsr_bwd_args *b, const nsr::RenderParams &P, void *stream) {
    const StageSlots st(P.stage);
    nsr::FinalParams R;
    R.stride = P.partial_stride; R.overwrite = b->overwrite_dparams ? 1 : 0;
    int rows = 0;
    for (int s = st.first; s <= st.last; ++s) {
        if (!P.dec[s].dparams) continue;
        const int pass = st.pass_of(s);
        nsr::FinalJob &J = R.job[rows++];
        J.images = P.partials + (long long)P.dw_beg[pass] * P.partial_stride;
        J.dbpart = P.dbpart + (long long)P.dx_beg[pass] * nsr::kDbPart;
        J.dparams = P.dec[s].dparams;
        J.kind = s; J.nimg = P.dw_beg[pass + 1] - P.dw_beg[pass]; J.ndx = P.dx_beg[pass + 1] - P.dx_beg[pass];
    }
    for (int r = rows; r < 3; ++r) R.job[r] = nsr::FinalJob{nullptr, nullptr, nullptr, 0, 0, 0};
    const int nblocks = st.most([&](int s) { return P.dec[s].dparams ? (nsr::param_total(s) + 63) / 64 : 0; });
    NSR_LAUNCH(nsr::bwd_finalize_kernel, dim3(nblocks, rows), dim3(kFinThreads), kFinThreads * 4, stream, R);
}

// the backward as comp_bwd -> dX -> dW -> finalize over the activations the forward saved (nsr_bwd2.h)
int render_bwd_split(const nsr_render_args *a, const nsr_bwd_args *b, nsr::RenderParams &P, bool any_params, void *stream) {
    const SplitGeo G = split_geo(P.stage, P.n_rays, P.S, b->max_blocks);
    int dx_beg[4], dw_beg[4];
    if (int rc = bind_bwd(b, P, G, any_params)) return rc;
    if (int rc = deal_bwd(P, G, dx_beg, dw_beg)) return rc;
    if (b->ev_start) nsr::rt_record(b->ev_start, stream);
    launch_comp_bwd(a, b, P, stream);
    if (int rc = launch_dx(P, G, dx_beg, stream)) return rc;
    if (b->ev_dx_done) nsr::rt_record(b->ev_dx_done, stream);
    if (any_params) {
        if (int rc = launch_dw(P, dw_beg, stream)) return rc;
        if (b->ev_dw_done) nsr::rt_record(b->ev_dw_done, stream);
        launch_finalize(b, P, stream);
    }
    if (b->ev_stop) nsr::rt_record(b->ev_stop, stream);
    return finish("nsr_render_bwd(split)");
}

}  // namespace

extern "C" {

int nsr_version(void) { return NSR_VERSION; }
const char *nsr_last_error(void) { return g_err.c_str(); }

int64_t nsr_param_count(int slot) { return (slot < 0 || slot > 3) ? -1 : nsr::param_total(slot); }
int64_t nsr_packed_count(int slot) { return (slot < 0 || slot > 3) ? -1 : nsr::packed_buf_total(slot); }

int64_t nsr_acts_floats(int stage, int64_t n_rays, int n_samples_total) {
    if (stage < 0 || stage > 3 || n_rays < 0 || n_samples_total < 1 || n_samples_total > NSR_MAX_SAMPLES) return -1;
    nsr::RenderParams P;
    P.stage = stage; P.n_rays = n_rays; P.S = n_samples_total;
    return carve(describe_acts, P) / 4;
}

int64_t nsr_bwd_workspace_floats(int stage, int64_t n_rays, int n_samples_total, int max_blocks) {
    if (stage < 0 || stage > 3 || n_samples_total < 1 || n_samples_total > NSR_MAX_SAMPLES) return -1;
    return bwd_workspace(stage, split_geo(stage, n_rays, n_samples_total, max_blocks)).floats;
}

int nsr_pack_params(int slot, const float *params, float *packed, void *stream) {
    if (slot < 0 || slot > 3) return fail("nsr_pack_params: slot out of range");
    if (!params || !packed) return fail("nsr_pack_params: null pointer");
    const int tb = 256;
    with_stage(slot, [&](auto SLOT) {
        NSR_LAUNCH(nsr::pack_kernel<SLOT()>, dim3(nblk(nsr::packed_buf_total(slot), tb)), dim3(tb), 0, stream, params, packed);
        return 0;
    });
    return finish("nsr_pack_params");
}

// sample placement -> decoder passes -> compositor (nsr_fwd2.h), saving into the activation buffer
static int render_fwd_split(const nsr_render_args *a, nsr::RenderParams &P, void *stream) {
    // one block per CU over all passes, dealt in proportion to the measured cost of a tile; waves per block from the largest tile
    // share, at most nsr::kDxMaxWaves (launch policy above)
    const StageSlots st(P.stage);
    const int wgt[3] = {kFwdWeight, fwd_fine_weight(P.stage), kFwdWeight};
    deal_blocks(P.pass_beg, kDefaultBwdBlocks, wgt, st.passes, P.act_tiles, false);
    long long most = 1;           // tiles of a block
    for (int p = 0; p < st.passes; ++p) most = std::max(most, (P.act_tiles + P.pass_beg[p + 1] - P.pass_beg[p] - 1) / (P.pass_beg[p + 1] - P.pass_beg[p]));
    const int waves = (int)std::min<long long>(most, nsr::kDxMaxWaves), rpb = 4;
    const dim3 rgrid(nblk(P.n_rays, rpb)), rblock(64 * rpb);
    NSR_LAUNCH(nsr::fwd_sample_kernel, rgrid, rblock, rpb * 64 * 8, stream, P);
    const int rc = with_stage(P.stage, [&](auto ST) {
        if (a->ev_pass_start) nsr::rt_record(a->ev_pass_start, stream);
        if (int rc = launch_kernel(nsr::render_fwd_pass_kernel<ST(), true>, dim3(P.pass_beg[3]), dim3(64 * waves), pass_lds_bytes(P.stage), "nsr_render_fwd(pass)", stream, P))
            return rc;
        if (a->ev_pass_stop) nsr::rt_record(a->ev_pass_stop, stream);
        NSR_LAUNCH(nsr::fwd_composite_kernel<ST()>, rgrid, rblock, rpb * 8, stream, P);
        return 0;
    });
    return rc ? rc : finish("nsr_render_fwd(split)");
}

int nsr_render_fwd(const nsr_render_args *a, void *stream) {
    nsr::RenderParams P;
    if (int rc = build_params(a, P, true)) return rc;
#ifdef NSR_TS
    if (const char *e = getenv("NSR_DBG_FWD_PTR")) P.dbg = reinterpret_cast<long long *>(strtoull(e, nullptr, 16));
#endif
    if (!a->depth || !a->var || !a->rgb) return fail("nsr_render_fwd: null output pointer");
    if (P.n_rays == 0) return 0;
    if (a->acts && a->zvals && a->raw) {
        // a call that hands over an activation buffer (with zvals and raw: without them nsr_render_bwd refuses) will be differentiated:
        // only the three-launch path saves into it, and the tile / keep arithmetic of the kernels that read it is 32-bit
        // (tile_live, dw_live_mask, describe_acts)
        if (P.n_points_total > (1ll << 25) - 16) return fail("nsr_render_fwd: more than 2^25 sample points in one differentiated call (split the ray batch)");
        return render_fwd_split(a, P, stream);
    }
    // (the one-launch kernel saves nothing: a call that will be differentiated passes acts + zvals + raw and took the branch above)
    P.acts = nullptr;
    const int lds = fwd_lds_bytes(P.stage, P.rays_per_block * P.S * (8 + 8 + 16));
    const dim3 grid((unsigned)(P.n_groups < (1 << 20) ? P.n_groups : (1 << 20))), block(64 * P.tiles_per_block);
    const int rc = with_stage(P.stage, [&](auto ST) { return launch_kernel(nsr::render_fwd_kernel<ST()>, grid, block, lds, "nsr_render_fwd", stream, P); });
    return rc ? rc : finish("nsr_render_fwd");
}

int nsr_render_bwd(const nsr_render_args *a, const nsr_bwd_args *b, void *stream) {
    nsr::RenderParams P;
    if (int rc = build_params(a, P, true, true)) return rc;
    if (!b) return fail("nsr_render_bwd: null backward block");
    if (!a->raw) return fail("nsr_render_bwd: the forward pass must have saved `raw`");
    if (!b->d_depth && !b->d_var && !b->d_rgb) return fail("nsr_render_bwd: no output gradient given");
    if (!b->depth) return fail("nsr_render_bwd: forward depth is required");
    if ((b->d_rays_o == nullptr) != (b->d_rays_d == nullptr)) return fail("nsr_render_bwd: d_rays_o / d_rays_d must be given together");
    if (P.n_rays == 0) return 0;
    P.d_depth = b->d_depth; P.d_var = b->d_var; P.d_rgb = b->d_rgb; P.g_depth = b->depth; P.g_scale = b->grad_scale;
    P.d_rays_o = b->d_rays_o; P.d_rays_d = b->d_rays_d;
#ifdef NSR_TS
    if (const char *e = getenv("NSR_DBG_PTR")) P.dbg = reinterpret_cast<long long *>(strtoull(e, nullptr, 16));
#endif
    bool any_params = false;
    for (int s = 0; s < 4; ++s) any_params |= P.dec[s].dparams != nullptr;
    P.partial_stride = partial_stride(P.stage);
    if (!P.acts || !a->zvals)
        return fail("nsr_render_bwd: the forward must have been given an activation buffer (nsr_render_args.acts, sized by nsr_acts_floats) and zvals");
    return render_bwd_split(a, b, P, any_params, stream);
}

int nsr_eval_points_fwd(const nsr_render_args *a, const double *points, int64_t n_points, float *out, void *stream) {
    nsr::RenderParams P;
    if (int rc = build_params(a, P, false)) return rc;
    if (n_points < 0 || (n_points > 0 && (!points || !out))) return fail("nsr_eval_points_fwd: bad points / out");
    if (n_points == 0) return 0;
    P.points = points; P.n_points = n_points; P.out_points = out;
    const int waves = kMaxTiles;
    long long nb = (tiles_of(n_points) + waves - 1) / waves;
    if (nb > 2048) nb = 2048;
    const int rc = with_stage(P.stage, [&](auto ST) {
        return launch_kernel(nsr::eval_points_kernel<ST()>, dim3((unsigned)nb), dim3(64 * waves), fwd_lds_bytes(P.stage, 16), "nsr_eval_points_fwd", stream, P);
    });
    return rc ? rc : finish("nsr_eval_points_fwd");
}

int nsr_masked_adam(float *p, const float *g, float *m, float *v, const uint8_t *voxel_mask, int64_t n_voxels,
                    float step_size, float beta1, float beta2, float eps, float bias2_sqrt, void *stream) {
    if (n_voxels < 0) return fail("nsr_masked_adam: negative voxel count");
    if (n_voxels == 0) return 0;
    if (!p || !g || !m || !v) return fail("nsr_masked_adam: null pointer");
    if (!(bias2_sqrt > 0.f)) return fail("nsr_masked_adam: bias2_sqrt must be positive (step >= 1)");
    nsr::AdamParams A;
    A.p = p; A.g = g; A.m = m; A.v = v; A.mask = voxel_mask; A.n_vox = n_voxels;
    A.step = step_size; A.b1 = beta1; A.b2 = beta2; A.eps = eps; A.rs2 = bias2_sqrt;
    const int tb = 256;
    const long long nthreads = n_voxels * 8;
    NSR_LAUNCH(nsr::masked_adam_kernel, dim3((unsigned)((nthreads + tb - 1) / tb)), dim3(tb), 0, stream, A);
    return finish("nsr_masked_adam");
}

int nsr_get_samples(const int64_t *indices, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                    int32_t W_full, float fx, float fy, float cx, float cy,
                    const float *c2w, int32_t c2w_stride, const float *depth, const float *color,
                    float *rays_o, float *rays_d, float *out_depth, float *out_color, void *stream) {
    if (n < 0 || H1 <= H0 || W1 <= W0 || W_full < W1) return fail("nsr_get_samples: bad crop");
    if (n == 0) return 0;
    if (!indices || !c2w || !depth || !color || !rays_o || !rays_d || !out_depth || !out_color)
        return fail("nsr_get_samples: null pointer");
    nsr::SampleParams S;
    S.indices = reinterpret_cast<const long long *>(indices);
    S.n = n; S.H0 = H0; S.W0 = W0; S.crop_w = W1 - W0; S.W_full = W_full;
    S.fx = fx; S.fy = fy; S.cx = cx; S.cy = cy;
    S.c2w = c2w; S.c2w_stride = c2w_stride; S.depth = depth; S.color = color;
    S.rays_o = rays_o; S.rays_d = rays_d; S.out_depth = out_depth; S.out_color = out_color;
    const int tb = 256;
    NSR_LAUNCH(nsr::get_samples_kernel, dim3((unsigned)((n + tb - 1) / tb)), dim3(tb), 0, stream, S);
    return finish("nsr_get_samples");
}

int64_t nsr_frustum_workspace_floats(int64_t n_voxels) {
    return n_voxels < 0 ? -1 : n_voxels + (n_voxels + 255) / 256;
}

int nsr_frustum_mask(const float *w2c, const float *cam_center, double fx, double fy, double cx, double cy,
                     int32_t H, int32_t W, const float *depth, const float *xs, const float *ys, const float *zs,
                     int32_t nx, int32_t ny, int32_t nz, float *workspace, uint8_t *voxel_mask, void *stream) {
    if (nx < 0 || ny < 0 || nz < 0 || H <= 0 || W <= 0) return fail("nsr_frustum_mask: bad shape");
    const int64_t n_vox = (int64_t)nx * ny * nz;
    if (n_vox == 0) return 0;
    if (H > 32766 || W > 32766) return fail("nsr_frustum_mask: image larger than 32766 pixels per side");
    if (!w2c || !cam_center || !depth || !xs || !ys || !zs || !workspace || !voxel_mask)
        return fail("nsr_frustum_mask: null pointer");
    nsr::FrustumParams P;
    for (int i = 0; i < 12; ++i) P.w2c[i] = w2c[i];
    for (int i = 0; i < 3; ++i) P.cam_o[i] = cam_center[i];
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.H = H; P.W = W;
    P.depth = depth; P.xs = xs; P.ys = ys; P.zs = zs; P.nx = nx; P.ny = ny; P.nz = nz;
    const int tb = 256;
    P.nblocks = (int)((n_vox + tb - 1) / tb);
    P.n_vox = n_vox; P.ws = workspace; P.mask = voxel_mask;
    NSR_LAUNCH(nsr::frustum_mask_kernel<0>, dim3((unsigned)P.nblocks), dim3(tb), tb * sizeof(float), stream, P);
    NSR_LAUNCH(nsr::frustum_mask_kernel<1>, dim3((unsigned)P.nblocks), dim3(tb), tb * sizeof(float), stream, P);
    return finish("nsr_frustum_mask");
}

int nsr_keyframe_overlap(const int64_t *indices, int32_t n_rays, int32_t n_samples, const float *t_vals,
                         int32_t H, int32_t W, double fx, double fy, double cx, double cy, int32_t edge,
                         const float *c2w, int32_t c2w_stride, const float *depth,
                         const float *w2c, int32_t K, int32_t *counts, void *stream) {
    if (!indices || !t_vals || !c2w || !depth || (K > 0 && (!w2c || !counts))) return fail("nsr_keyframe_overlap: null pointer");
    if (K < 0) return fail("nsr_keyframe_overlap: K must be >= 0");
    if (n_rays < 1 || n_rays > (1 << 24)) return fail("nsr_keyframe_overlap: n_rays must be in [1, 2^24]");
    if (n_samples < 1 || n_samples > NSR_KF_MAX_SAMPLES) return fail("nsr_keyframe_overlap: n_samples must be in [1, 64]");
    if (H <= 0 || W <= 0 || H > 32766 || W > 32766) return fail("nsr_keyframe_overlap: bad image shape");
    if (edge < 0 || 2 * edge >= W || 2 * edge >= H) return fail("nsr_keyframe_overlap: edge must satisfy 0 <= 2 * edge < min(H, W)");
    if (c2w_stride < 4) return fail("nsr_keyframe_overlap: c2w_stride must be >= 4");
    if (K == 0) return 0;
    nsr::KeyframeParams P;
    std::memset(&P, 0, sizeof(P));
    P.indices = reinterpret_cast<const long long *>(indices);
    P.c2w = c2w; P.depth = depth; P.w2c = w2c; P.counts = counts;
    P.n_rays = n_rays; P.n_samples = n_samples; P.H = H; P.W = W; P.K = K; P.edge = edge; P.c2w_stride = c2w_stride;
    P.fx = (float)fx; P.fy = (float)fy; P.cx = (float)cx; P.cy = (float)cy;
    P.dfx = fx; P.dfy = fy; P.dcx = cx; P.dcy = cy;
    for (int i = 0; i < n_samples; ++i) P.t_vals[i] = t_vals[i];
    const int tb = NSR_KF_THREADS;
    const int blocks = K < kKeyframeBlocks ? K : kKeyframeBlocks;
    NSR_LAUNCH(nsr::keyframe_overlap_kernel, dim3((unsigned)blocks), dim3(tb), 3 * NSR_KF_CHUNK * sizeof(float) + (tb / 64) * sizeof(int),
               stream, P);
    return finish("nsr_keyframe_overlap");
}

}  // extern "C"
namespace {
int window_launch(const int64_t *indices, int64_t *indices_out, uint64_t *rng, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                  int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                  float *rays_o, float *rays_d, float *out_depth, float *out_color,
                  const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream,
                  float *hdr = nullptr, float *zero = nullptr, int64_t zero_floats = 0, const uint64_t *peer_seeds = nullptr, int32_t n_peers = 0) {
    if (K < 0 || K > NSR_MAX_WINDOW) return fail("nsr_get_samples_window: K must be in [0, 32]");
    if (n < 0 || H1 <= H0 || W1 <= W0 || W_full < W1) return fail("nsr_get_samples_window: bad crop");
    if (K == 0 || n == 0) return 0;
    if ((!indices && (!indices_out || !rng)) || !frames || !rays_o || !rays_d || !out_depth || !out_color || !bound_lo || !bound_hi)
        return fail("nsr_get_samples_window: null pointer");
    if ((long long)(H1 - H0) * (W1 - W0) >= (1ll << 32)) return fail("nsr_get_samples_window: crop too large");
    nsr::WindowParams P;
    std::memset(&P, 0, sizeof(P));
    P.indices = reinterpret_cast<const long long *>(indices);
    P.indices_out = reinterpret_cast<long long *>(indices_out);
    P.rng = reinterpret_cast<unsigned long long *>(rng);
    P.crop_pixels = (unsigned)((H1 - H0) * (W1 - W0));
    P.n = n; P.K = K; P.H0 = H0; P.W0 = W0; P.crop_w = W1 - W0; P.W_full = W_full;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy;
    for (int k = 0; k < K; ++k) {
        if (!frames[k].depth || !frames[k].color || !frames[k].c2w) return fail("nsr_get_samples_window: null frame pointer");
        P.depth[k] = frames[k].depth; P.color[k] = frames[k].color; P.c2w[k] = frames[k].c2w; P.c2w_stride[k] = frames[k].c2w_stride;
    }
    P.rays_o = rays_o; P.rays_d = rays_d; P.out_depth = out_depth; P.out_color = out_color;
    for (int a = 0; a < 3; ++a) { P.lo[a] = bound_lo[a]; P.hi[a] = bound_hi[a]; }
    P.keep = keep; P.kept_max = kept_max;
    const int tb = 256;
    const long long sbx = (n + tb - 1) / tb;
    P.sample_bx = (int)sbx;
    long long fbx = 0;
    if (hdr) {
        // fill blocks beside the sampling blocks: 32 KB each (eight 16-byte stores per thread), at most ~2048 over the K grid rows
        if (zero_floats < 0 || (zero_floats > 0 && (!zero || (reinterpret_cast<uintptr_t>(zero) & 15)))) return fail("nsr_get_samples_window_fused: zero span must be 16-byte aligned");
        P.hdr = hdr; P.zero = zero; P.zero_n = zero_floats;
        long long want = (zero_floats * 4 + 32767) / 32768;
        if (want > 2048) want = 2048;
        fbx = (want + K - 1) / K;
    }
    if (n_peers) {
        if (n_peers < 0 || n_peers > NSR_MAX_PEERS || !peer_seeds) return fail("nsr_get_samples_window_sharded: 0..15 peers");
        if (indices || !hdr) return fail("nsr_get_samples_window_sharded: peers need the in-kernel pixel draw (indices == NULL) and the fused header");
        P.n_peers = n_peers;
        for (int p = 0; p < n_peers; ++p) P.peer_seed[p] = peer_seeds[p];
    }
    NSR_LAUNCH(nsr::get_samples_window_kernel, dim3((unsigned)(sbx * (1 + n_peers) + fbx), K), dim3(tb), 0, stream, P);
    return finish("nsr_get_samples_window");
}
}  // namespace
extern "C" {

int nsr_get_samples_window(const int64_t *indices, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                           int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                           float *rays_o, float *rays_d, float *out_depth, float *out_color,
                           const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream) {
    if (!indices) return fail("nsr_get_samples_window: null pointer");
    return window_launch(indices, nullptr, nullptr, K, n, H0, H1, W0, W1, W_full, fx, fy, cx, cy, frames, rays_o, rays_d, out_depth, out_color,
                         bound_lo, bound_hi, keep, kept_max, stream);
}

int nsr_get_samples_window_draw(int64_t *indices_out, uint64_t *rng_state, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0,
                                int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                                float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream) {
    return window_launch(nullptr, indices_out, rng_state, K, n, H0, H1, W0, W1, W_full, fx, fy, cx, cy, frames, rays_o, rays_d, out_depth,
                         out_color, bound_lo, bound_hi, keep, kept_max, stream);
}

int nsr_get_samples_window_fused(const int64_t *indices, int64_t *indices_out, uint64_t *state, int32_t K, int64_t n, int32_t H0, int32_t H1,
                                 int32_t W0, int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                                 float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                 const double *bound_lo, const double *bound_hi, uint8_t *keep, float *header,
                                 float *zero, int64_t zero_floats, void *stream) {
    if (!state || !header) return fail("nsr_get_samples_window_fused: null pointer");
    if ((reinterpret_cast<uintptr_t>(header) & 15) || (reinterpret_cast<uintptr_t>(state) & 7))
        return fail("nsr_get_samples_window_fused: header must be 16-byte aligned (it is written with one 16-byte store), state 8-byte aligned");
    if (!indices && !indices_out) return fail("nsr_get_samples_window_fused: indices or indices_out is required");
    if (K == 0 || n == 0) return fail("nsr_get_samples_window_fused: empty window (the header and the zero span would stay unwritten)");
    return window_launch(indices, indices ? nullptr : indices_out, state, K, n, H0, H1, W0, W1, W_full, fx, fy, cx, cy, frames, rays_o, rays_d,
                         out_depth, out_color, bound_lo, bound_hi, keep, nullptr, stream, header, zero, zero_floats);
}

int nsr_get_samples_window_sharded(int64_t *indices_out, uint64_t *state, const uint64_t *peer_seeds, int32_t n_peers, int32_t K, int64_t n,
                                   int32_t H0, int32_t H1, int32_t W0, int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy,
                                   const nsr_frame *frames, float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                   const double *bound_lo, const double *bound_hi, uint8_t *keep, float *header,
                                   float *zero, int64_t zero_floats, void *stream) {
    if (!state || !header || !indices_out) return fail("nsr_get_samples_window_sharded: null pointer");
    if ((reinterpret_cast<uintptr_t>(header) & 15) || (reinterpret_cast<uintptr_t>(state) & 7)) return fail("nsr_get_samples_window_sharded: header must be 16-byte, state 8-byte aligned");
    if (K == 0 || n == 0) return fail("nsr_get_samples_window_sharded: empty window (the header and the zero span would stay unwritten)");
    return window_launch(nullptr, indices_out, state, K, n, H0, H1, W0, W1, W_full, fx, fy, cx, cy, frames, rays_o, rays_d,
                         out_depth, out_color, bound_lo, bound_hi, keep, nullptr, stream, header, zero, zero_floats, peer_seeds, n_peers);
}

int nsr_pose_grad(const int64_t *indices, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                  float fx, float fy, float cx, float cy, const float *d_rays_o, const float *d_rays_d,
                  float *d_c2w, int32_t out_stride, void *stream) {
    if (K < 0 || n < 0 || H1 <= H0 || W1 <= W0 || out_stride < 12) return fail("nsr_pose_grad: bad arguments");
    if (K == 0) return 0;
    if (!indices || !d_rays_o || !d_rays_d || !d_c2w) return fail("nsr_pose_grad: null pointer");
    nsr::PoseGradParams P;
    P.indices = reinterpret_cast<const long long *>(indices);
    P.n = n; P.H0 = H0; P.W0 = W0; P.crop_w = W1 - W0;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy;
    P.d_rays_o = d_rays_o; P.d_rays_d = d_rays_d; P.out = d_c2w; P.out_stride = out_stride;
    const int tb = 256;
    NSR_LAUNCH(nsr::pose_grad_kernel, dim3((unsigned)K), dim3(tb), 12 * tb * sizeof(float), stream, P);
    return finish("nsr_pose_grad");
}

int nsr_masked_adam_multi(const nsr_adam_grid *grids, int32_t n_grids, double beta1, double beta2, double eps,
                          int32_t zero_grad, float *scratch, void *stream) {
    if (n_grids < 0 || n_grids > 4) return fail("nsr_masked_adam_multi: 0..4 grids");
    if (n_grids == 0) return 0;
    if (!grids || !scratch) return fail("nsr_masked_adam_multi: null pointer");
    nsr::AdamMulti A;
    std::memset(&A, 0, sizeof(A));
    long long nmax = 0;
    for (int i = 0; i < n_grids; ++i) {
        const nsr_adam_grid &g = grids[i];
        if (!g.p || !g.g || !g.m || !g.v || !g.step || g.n_voxels < 0) return fail("nsr_masked_adam_multi: bad grid entry");
        A.p[i] = g.p; A.g[i] = g.g; A.m[i] = g.m; A.v[i] = g.v; A.mask[i] = g.voxel_mask; A.n_vox[i] = g.n_voxels;
        A.step[i] = g.step; A.lr[i] = g.lr;
        nmax = g.n_voxels > nmax ? g.n_voxels : nmax;
    }
    A.n = n_grids; A.b1 = (float)beta1; A.b2 = (float)beta2; A.eps = (float)eps; A.zero_grad = zero_grad; A.scal = scratch;
    A.b1d = beta1; A.b2d = beta2;
    NSR_LAUNCH(nsr::adam_tick_kernel, dim3(1), dim3(64), 0, stream, A);
    if (nmax > 0) {
        const int tb = 256;
        NSR_LAUNCH(nsr::masked_adam_multi_kernel, dim3((unsigned)((nmax * 8 + tb - 1) / tb), n_grids), dim3(tb), 0, stream, A);
    }
    return finish("nsr_masked_adam_multi");
}

int nsr_flat_adam(const nsr_adam_span *spans, int32_t n_spans, double beta1, double beta2, double eps, int32_t zero_grad, float *scratch,
                  void *stream) {
    if (n_spans < 0 || n_spans > 4) return fail("nsr_flat_adam: 0..4 spans");
    if (n_spans == 0) return 0;
    if (!spans || !scratch) return fail("nsr_flat_adam: null pointer");
    nsr::AdamMulti A;
    std::memset(&A, 0, sizeof(A));
    long long nmax = 0;
    for (int i = 0; i < n_spans; ++i) {
        const nsr_adam_span &g = spans[i];
        if (!g.p || !g.g || !g.m || !g.v || !g.step || g.n < 0) return fail("nsr_flat_adam: bad span entry");
        A.p[i] = g.p; A.g[i] = g.g; A.m[i] = g.m; A.v[i] = g.v; A.n_vox[i] = g.n; A.step[i] = g.step; A.lr[i] = g.lr;
        nmax = g.n > nmax ? g.n : nmax;
    }
    A.n = n_spans; A.b1 = (float)beta1; A.b2 = (float)beta2; A.eps = (float)eps; A.zero_grad = zero_grad; A.scal = scratch;
    A.omb1 = (float)(1.0 - beta1); A.omb2 = (float)(1.0 - beta2);
    A.b1d = beta1; A.b2d = beta2;
    NSR_LAUNCH(nsr::adam_tick_kernel, dim3(1), dim3(64), 0, stream, A);
    if (nmax > 0) {
        const int tb = 256;
        NSR_LAUNCH(nsr::flat_adam_kernel, dim3((unsigned)((nmax + tb - 1) / tb), n_spans), dim3(tb), 0, stream, A);
    }
    return finish("nsr_flat_adam");
}

int nsr_pack_rows(const nsr_rows *grids, int32_t n_grids, const nsr_span *spans, int32_t n_spans, float *packed,
                  int32_t unpack, void *stream) {
    if (n_grids < 0 || n_grids > 4 || n_spans < 0 || n_spans > 4) return fail("nsr_pack_rows: at most 4 grids and 4 spans");
    if ((n_grids && !grids) || (n_spans && !spans) || !packed) return fail("nsr_pack_rows: null pointer");
    nsr::PackParams P;
    std::memset(&P, 0, sizeof(P));
    long long total = 0;
    for (int i = 0; i < n_grids; ++i) {
        if (grids[i].n_rows < 0 || (grids[i].n_rows && (!grids[i].grid || !grids[i].rows))) return fail("nsr_pack_rows: bad grid entry");
        P.grid[i] = grids[i].grid; P.rows[i] = reinterpret_cast<const long long *>(grids[i].rows); P.n_rows[i] = grids[i].n_rows;
        total += grids[i].n_rows * nsr::kC;
    }
    for (int i = 0; i < n_spans; ++i) {
        if (spans[i].n < 0 || (spans[i].n && !spans[i].ptr)) return fail("nsr_pack_rows: bad span entry");
        P.span[i] = spans[i].ptr; P.span_n[i] = spans[i].n;
        total += spans[i].n;
    }
    P.n_grids = n_grids; P.n_spans = n_spans; P.unpack = unpack ? 1 : 0; P.packed = packed; P.total = total;
    if (total == 0) return 0;
    const int tb = 256;
    NSR_LAUNCH(nsr::pack_rows_kernel, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, stream, P);
    return finish("nsr_pack_rows");
}

int nsr_aabb_keep(const float *rays_o, const float *rays_d, const float *gt_depth, int64_t n,
                  const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream) {
    if (n < 0) return fail("nsr_aabb_keep: negative ray count");
    if (n == 0) return 0;
    if (!rays_o || !rays_d || !gt_depth || !bound_lo || !bound_hi || !keep) return fail("nsr_aabb_keep: null pointer");
    nsr::AabbParams P;
    P.rays_o = rays_o; P.rays_d = rays_d; P.gt_depth = gt_depth; P.n = n;
    for (int a = 0; a < 3; ++a) { P.lo[a] = bound_lo[a]; P.hi[a] = bound_hi[a]; }
    P.keep = keep; P.kept_max = kept_max;
    const int tb = 256;
    NSR_LAUNCH(nsr::aabb_keep_kernel, dim3((unsigned)((n + tb - 1) / tb)), dim3(tb), 0, stream, P);
    return finish("nsr_aabb_keep");
}

int nsr_tracking_loss(int64_t n_rays, const float *gt_depth, const float *gt_color, const uint8_t *keep,
                      const double *depth, const double *var, const float *rgb,
                      int32_t handle_dynamic, int32_t use_color, float w_color,
                      double *loss, double *dl_depth, float *dl_rgb, void *stream) {
    if (n_rays < 0) return fail("nsr_tracking_loss: negative ray count");
    if (n_rays == 0) return 0;
    if (!gt_depth || !depth || !var || !loss || !dl_depth) return fail("nsr_tracking_loss: null pointer");
    if (use_color && (!gt_color || !rgb || !dl_rgb)) return fail("nsr_tracking_loss: the colour term needs gt_color, rgb and dl_rgb");
    nsr::TrackLossParams P;
    P.n = n_rays; P.gt_depth = gt_depth; P.gt_color = gt_color; P.rgb = rgb; P.keep = keep; P.depth = depth; P.var = var;
    P.handle_dynamic = handle_dynamic ? 1 : 0; P.use_color = use_color ? 1 : 0; P.w_color = w_color;
    P.loss = loss; P.dl_depth = dl_depth; P.dl_rgb = dl_rgb;
    const int tb = n_rays <= 256 ? 256 : 1024;                       // one block: the median is a property of the whole batch
    const int key_cap = (handle_dynamic && n_rays <= 4096) ? (int)n_rays : 0;      // tmp bit patterns cached in LDS (<= 32 KB), else recomputed
    // (key slots for every thread of the block: the one-ray-per-thread path of n <= tb pads the key list with skip marks)
    NSR_LAUNCH(nsr::tracking_loss_kernel, dim3(1), dim3(tb), 1024 + 32 + tb * 8 + (key_cap > 0 && key_cap < tb ? tb : key_cap) * 8, stream, P, key_cap);
    return finish("nsr_tracking_loss");
}

int nsr_camera_from_tensor(const float *cam, int64_t n, float *rt, const float *d_rt, float *d_cam, void *stream) {
    if (n < 0) return fail("nsr_camera_from_tensor: negative count");
    if (n == 0) return 0;
    if (!cam || (!d_rt && !rt) || (d_rt && !d_cam)) return fail("nsr_camera_from_tensor: null pointer");
    nsr::CamParams P;
    P.cam = cam; P.n = n; P.rt = rt; P.d_rt = d_rt; P.d_cam = d_cam;
    const int tb = 64;
    NSR_LAUNCH(nsr::camera_from_tensor_kernel, dim3((unsigned)((n + tb - 1) / tb)), dim3(tb), 0, stream, P);
    return finish("nsr_camera_from_tensor");
}

}  // extern "C"

// ---- mesh extraction (include/nsr.h, "Mesh extraction") ----
namespace {
constexpr int kMcThreads = 256;

// the lattice's sizes into P; false: a lattice the kernels do not take
bool mc_sizes(nsr::McParams &P, int32_t nx, int32_t ny, int32_t nz) {
    std::memset(&P, 0, sizeof(P));
    if (nx < 2 || ny < 2 || nz < 2) return false;
    P.nx = nx; P.ny = ny; P.nz = nz; P.n = (long long)nx * ny * nz;
    if (P.n > (1ll << 31)) return false;
    P.nblocks = (int)((P.n + kMcThreads - 1) / kMcThreads);
    return true;
}

void mc_carve(nsr::McParams &P, Carve &c) {
    P.code = c.take<unsigned char>(P.n);
    P.voff = c.take<int>(P.n);
    P.blk = c.take<long long>(2ll * P.nblocks);
}

int mc_setup(nsr::McParams &P, const float *vol, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace, const char *what) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(std::string(what) + ": every lattice dimension must be at least 2");
    if (!mc_sizes(P, nx, ny, nz)) return fail(std::string(what) + ": lattice larger than 2^31 points");
    if (!vol || !workspace) return fail(std::string(what) + ": null pointer");
    P.vol = vol; P.level = level;
    carve(mc_carve, P, workspace);
    return 0;
}
}  // namespace

extern "C" {

int64_t nsr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    nsr::McParams P;
    if (!mc_sizes(P, nx, ny, nz)) return -1;
    return carve(mc_carve, P);
}

int nsr_mc_count(const float *vol, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace, int64_t *counts, void *stream) {
    nsr::McParams P;
    if (int rc = mc_setup(P, vol, nx, ny, nz, level, workspace, "nsr_mc_count")) return rc;
    if (!counts) return fail("nsr_mc_count: null pointer");
    P.counts = reinterpret_cast<long long *>(counts);
    NSR_LAUNCH(nsr::mc_count_kernel, dim3((unsigned)P.nblocks), dim3(kMcThreads), kMcThreads * 4, stream, P);
    NSR_LAUNCH(nsr::mc_scan_kernel, dim3(1), dim3(1024), 2 * 1024 * 8, stream, P);
    return finish("nsr_mc_count");
}

int nsr_mc_emit(const float *vol, int32_t nx, int32_t ny, int32_t nz, float level, const double *origin, const double *spacing,
                void *workspace, int64_t n_verts, int64_t n_faces, double *verts, int32_t *faces, void *stream) {
    nsr::McParams P;
    if (int rc = mc_setup(P, vol, nx, ny, nz, level, workspace, "nsr_mc_emit")) return rc;
    if (n_verts < 0 || n_faces < 0) return fail("nsr_mc_emit: negative count");
    if (n_verts > 2147483647ll || 3 * n_faces > 2147483647ll) return fail("nsr_mc_emit: vertex or face index count does not fit in int32");
    if (!origin || !spacing || (n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return fail("nsr_mc_emit: null pointer");
    if (n_verts == 0) return 0;
    for (int k = 0; k < 3; ++k) { P.origin[k] = origin[k]; P.spacing[k] = spacing[k]; }
    P.verts = verts; P.faces = faces;
    NSR_LAUNCH(nsr::mc_emit_verts_kernel, dim3((unsigned)P.nblocks), dim3(kMcThreads), kMcThreads * 4, stream, P);
    if (n_faces > 0) NSR_LAUNCH(nsr::mc_emit_faces_kernel, dim3((unsigned)P.nblocks), dim3(kMcThreads), kMcThreads * 4, stream, P);
    return finish("nsr_mc_emit");
}

int64_t nsr_point_masks_workspace_floats(int64_t n, int64_t chunk, int32_t K) {
    if (n < 0 || chunk < 1 || K < 0) return -1;
    return ((n + chunk - 1) / chunk) * K;
}

int nsr_point_masks(const float *points, int64_t n, int64_t chunk, int32_t mode, int32_t K, const float *w2c, const float *depth,
                    const float *limit, int32_t H, int32_t W, double fx, double fy, double cx, double cy, float *workspace,
                    uint8_t *out, void *stream) {
    if (n < 0 || chunk < 1 || K < 0) return fail("nsr_point_masks: negative count or chunk < 1");
    if (mode < 0 || mode > 2) return fail("nsr_point_masks: mode must be 0 (all frames), 1 (keyframes) or 2 (keyframes, depth test)");
    if (H < 2 || W < 2) return fail("nsr_point_masks: image must be at least 2 x 2");
    if (n == 0) return 0;
    if (!points || !out || (K > 0 && !w2c)) return fail("nsr_point_masks: null pointer");
    if (K > 0 && mode == 1 && !limit) return fail("nsr_point_masks: mode 1 needs the per-keyframe depth limits");
    if (K > 0 && mode == 2 && (!depth || !workspace)) return fail("nsr_point_masks: mode 2 needs the keyframe depths and a workspace");
    nsr::MaskParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = points; P.n = n; P.chunk = chunk; P.nchunks = (n + chunk - 1) / chunk;
    P.K = K; P.mode = mode; P.H = H; P.W = W;
    const double km[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) P.kf[i] = (float)km[i];
    P.w2c = w2c; P.depth = depth; P.limit = limit; P.cmax = workspace; P.out = out;
    const int tb = 256;
    const dim3 grid((unsigned)((n + tb - 1) / tb));
    if (K > 0 && mode == 2) {
        NSR_LAUNCH(nsr::point_mask_kernel<0>, dim3((unsigned)((P.nchunks * K + tb - 1) / tb)), dim3(tb), 0, stream, P);
        NSR_LAUNCH(nsr::point_mask_kernel<1>, grid, dim3(tb), 0, stream, P);
    }
    NSR_LAUNCH(nsr::point_mask_kernel<2>, grid, dim3(tb), 0, stream, P);
    return finish("nsr_point_masks");
}

int nsr_cc_init(int64_t n, uint32_t *parent, uint32_t *changed, void *stream) {
    if (n < 0 || n >= (1ll << 32) - 1) return fail("nsr_cc_init: element count out of range");
    if (!parent || !changed) return fail("nsr_cc_init: null pointer");
    nsr::CcParams P;
    std::memset(&P, 0, sizeof(P));
    P.n = n; P.parent = parent; P.changed = changed;
    NSR_LAUNCH(nsr::cc_init_kernel, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, stream, P);
    return finish("nsr_cc_init");
}

int nsr_cc_round(const int32_t *pairs, int64_t n_pairs, int64_t n, uint32_t *parent, uint32_t *changed, int32_t round, void *stream) {
    if (n < 0 || n >= (1ll << 32) - 1 || n_pairs < 0 || round < 0) return fail("nsr_cc_round: count or round out of range");
    if (!parent || !changed || (n_pairs > 0 && !pairs)) return fail("nsr_cc_round: null pointer");
    if (n == 0) return 0;
    nsr::CcParams P;
    std::memset(&P, 0, sizeof(P));
    P.pairs = pairs; P.n_pairs = n_pairs; P.n = n; P.parent = parent; P.changed = changed; P.round = (unsigned)round + 1u;
    if (n_pairs > 0) NSR_LAUNCH(nsr::cc_hook_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::cc_jump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, P);
    return finish("nsr_cc_round");
}

int nsr_face_areas(const double *verts, const int32_t *faces, int64_t n_faces, double *area, void *stream) {
    if (n_faces < 0) return fail("nsr_face_areas: negative count");
    if (n_faces == 0) return 0;
    if (!verts || !faces || !area) return fail("nsr_face_areas: null pointer");
    nsr::CcParams P;
    std::memset(&P, 0, sizeof(P));
    P.verts = verts; P.faces = faces; P.n = n_faces; P.area = area;
    NSR_LAUNCH(nsr::face_area_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, stream, P);
    return finish("nsr_face_areas");
}

int nsr_segment_sums(const double *values, const int64_t *order, const int64_t *keys, int64_t n, const int64_t *seg, int64_t n_seg,
                     double *partial, double *out, void *stream) {
    if (n < 0 || n_seg < 0) return fail("nsr_segment_sums: negative count");
    if (n_seg == 0) return 0;
    if (!values || !order || !keys || !seg || !partial || !out) return fail("nsr_segment_sums: null pointer");
    nsr::CcParams P;
    std::memset(&P, 0, sizeof(P));
    P.area = const_cast<double *>(values); P.order = reinterpret_cast<const long long *>(order);
    P.keys = reinterpret_cast<const long long *>(keys); P.n = n; P.partial = partial;
    P.seg = reinterpret_cast<const long long *>(seg); P.n_seg = n_seg; P.seg_area = out;
    if (n > 0) NSR_LAUNCH(nsr::segment_partial_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::segment_area_kernel, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, stream, P);
    return finish("nsr_segment_sums");
}

}  // extern "C"

// ---- reconstruction evaluation (include/nsr.h, "Reconstruction evaluation") ----
namespace {

// the four run tables of a grid inside an index's workspace
void carve_runs(Carve &c, nsr::NnGrid &G) {
    G.fstart = c.take<int>(G.ncell);
    G.fend = c.take<int>(G.ncell);
    G.cstart = c.take<int>(G.ncoarse);
    G.cend = c.take<int>(G.ncoarse);
}

// workspace of nsr_nn_build / nsr_nn_query
void nn_carve(nsr::NnParams &P, Carve &c) {
    P.sref = c.take<double>(3 * P.m);
    P.sidx = c.take<long long>(P.m);
    carve_runs(c, P.G);
    P.cbox = c.take<double>(6 * P.G.ncoarse);
}

// the plan as a grid (its run tables unbound); false if it is not one nsr_nn_plan could have written for m points (m < 0: for
// any number of points)
bool grid_from_plan(nsr::NnGrid &G, const double *plan, long long m) {
    std::memset(&G, 0, sizeof(G));
    if (!plan || m == 0) return false;
    for (int d = 0; d < 3; ++d) {
        G.lo[d] = plan[nsr::kNnLo + d];
        G.hi[d] = plan[nsr::kNnHi + d];
        const double n = plan[nsr::kNnDim + d], c = plan[nsr::kNnCDim + d];
        if (!(n >= 1 && n <= (1 << 20) && c == std::ceil(n / nsr::kNnLocal))) return false;
        G.nd[d] = (int)n;
        G.nc[d] = (int)c;
        if (!std::isfinite(G.lo[d]) || !std::isfinite(G.hi[d])) return false;
    }
    G.h = plan[nsr::kNnH];
    G.slack = plan[nsr::kNnSlack];
    G.ncell = (long long)G.nd[0] * G.nd[1] * G.nd[2];
    G.ncoarse = (long long)G.nc[0] * G.nc[1] * G.nc[2];
    return G.h > 0 && std::isfinite(G.h) && G.ncell == (long long)plan[nsr::kNnCells] && G.ncoarse == (long long)plan[nsr::kNnCoarse] &&
           (m < 0 || G.ncell <= 4 * m + 64);
}

// NnParams for m reference points over the plan's grid; false as grid_from_plan
bool nn_from_plan(nsr::NnParams &P, const double *plan, long long m) {
    std::memset(&P, 0, sizeof(P));
    P.m = m;
    return grid_from_plan(P.G, plan, m);
}

}  // namespace

extern "C" {

int nsr_nn_bounds(const void *ref, int64_t n_ref, int32_t fp64, double *bounds, void *stream) {
    if (n_ref < 1) return fail("nsr_nn_bounds: the reference set is empty");
    if (!ref || !bounds) return fail("nsr_nn_bounds: null pointer");
    nsr::NnParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = ref; P.n = n_ref; P.fp64 = fp64 ? 1 : 0; P.bounds = bounds;
    NSR_LAUNCH(nsr::nn_bounds_kernel, dim3(nsr::kNnBoundBlocks), dim3(256), 6 * 256 * 8, stream, P);
    NSR_LAUNCH(nsr::nn_bounds_final_kernel, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_nn_bounds");
}

int nsr_nn_plan(const double *bounds, int64_t n_ref, double *plan) {
    if (n_ref < 1 || n_ref >= 2147483647ll) return fail("nsr_nn_plan: the reference set must hold 1 .. 2^31 - 2 points");
    if (!bounds || !plan) return fail("nsr_nn_plan: null pointer");
    double ext[3], emax = 0.0, amax = 0.0;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(bounds[d]) || !std::isfinite(bounds[3 + d]) || bounds[3 + d] < bounds[d])
            return fail("nsr_nn_plan: non-finite reference coordinates");
        ext[d] = bounds[3 + d] - bounds[d];
        emax = ext[d] > emax ? ext[d] : emax;
        amax = std::fmax(amax, std::fmax(std::fabs(bounds[d]), std::fabs(bounds[3 + d])));
    }
    // about 2 cells per reference point over the extents that are not degenerate (a plane or a line gets a 2-D or 1-D grid)
    const double target = 2.0 * (double)n_ref, cap = 4.0 * (double)n_ref + 64.0;
    double prod = 1.0;
    int k = 0;
    bool active[3];
    for (int d = 0; d < 3; ++d) {
        active[d] = emax > 0.0 && ext[d] > 1e-9 * emax;
        if (active[d]) { prod *= ext[d]; ++k; }
    }
    double h = k ? std::pow(prod / target, 1.0 / k) : 1.0;
    if (!(h > 0.0) || !std::isfinite(h)) h = emax > 0.0 ? emax : 1.0;
    double n[3];
    for (int it = 0;; ++it) {
        double cells = 1.0;
        bool fits = true;
        for (int d = 0; d < 3; ++d) {
            n[d] = active[d] ? std::fmax(1.0, std::ceil(ext[d] / h)) : 1.0;
            fits = fits && n[d] <= (double)(1 << 20);
            cells *= n[d];
        }
        if (fits && cells <= cap) break;
        if (it > 400) return fail("nsr_nn_plan: no grid of O(n_ref) cells covers the reference set");
        h *= 1.05;
    }
    for (int d = 0; d < 3; ++d) {
        plan[nsr::kNnLo + d] = bounds[d];
        plan[nsr::kNnHi + d] = bounds[3 + d];
        plan[nsr::kNnDim + d] = n[d];
        plan[nsr::kNnCDim + d] = std::ceil(n[d] / nsr::kNnLocal);
    }
    plan[nsr::kNnH] = h;
    plan[nsr::kNnCells] = n[0] * n[1] * n[2];
    plan[nsr::kNnCoarse] = plan[nsr::kNnCDim] * plan[nsr::kNnCDim + 1] * plan[nsr::kNnCDim + 2];
    plan[nsr::kNnSlack] = 1e-12 * (amax + emax + h);    // rounding of cell positions and distances, far above the few ulps it covers
    return 0;
}

int64_t nsr_nn_workspace_bytes(const double *plan, int64_t n_ref) {
    nsr::NnParams P;
    if (!nn_from_plan(P, plan, n_ref)) return -1;
    return carve(nn_carve, P);
}

int nsr_nn_keys(const void *pts, int64_t n, int32_t fp64, const double *plan, int64_t *keys, void *stream) {
    nsr::NnParams P;
    if (n < 0) return fail("nsr_nn_keys: negative count");
    if (!nn_from_plan(P, plan, -1)) return fail("nsr_nn_keys: invalid plan");
    if (n == 0) return 0;
    if (!pts || !keys) return fail("nsr_nn_keys: null pointer");
    P.pts = pts; P.n = n; P.fp64 = fp64 ? 1 : 0; P.keys = reinterpret_cast<long long *>(keys);
    NSR_LAUNCH(nsr::nn_keys_kernel, dim3(nblk(n, 256)), dim3(256), 0, stream, P);
    return finish("nsr_nn_keys");
}

int nsr_nn_build(const void *ref, int64_t n_ref, int32_t fp64, const double *plan, const int64_t *sorted_keys, const int64_t *order,
                 void *workspace, void *stream) {
    nsr::NnParams P;
    if (!nn_from_plan(P, plan, n_ref)) return fail("nsr_nn_build: invalid plan for this reference set");
    if (!ref || !sorted_keys || !order || !workspace) return fail("nsr_nn_build: null pointer");
    carve(nn_carve, P, workspace);
    P.pts = ref; P.n = n_ref; P.fp64 = fp64 ? 1 : 0;
    P.keys = const_cast<long long *>(reinterpret_cast<const long long *>(sorted_keys));
    P.order = reinterpret_cast<const long long *>(order);
    const long long nclear = P.G.ncell > P.G.ncoarse ? P.G.ncell : P.G.ncoarse;
    NSR_LAUNCH(nsr::nn_clear_kernel, dim3(nblk(nclear, 256)), dim3(256), 0, stream, P.G);
    NSR_LAUNCH(nsr::nn_gather_kernel, dim3(nblk(n_ref, 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::nn_box_kernel, dim3(nblk(P.G.ncoarse, 64)), dim3(64), 0, stream, P);
    return finish("nsr_nn_build");
}

int nsr_nn_query(const void *query, int64_t n_query, int32_t fp64, const int64_t *qorder, const double *plan, const void *workspace,
                 int64_t n_ref, double *dist, int64_t *idx, int32_t *ncand, void *stream) {
    nsr::NnParams P;
    if (n_query < 0) return fail("nsr_nn_query: negative count");
    if (!nn_from_plan(P, plan, n_ref)) return fail("nsr_nn_query: invalid plan for this reference set");
    if (n_query == 0) return 0;
    if (!query || !workspace || !dist || !idx) return fail("nsr_nn_query: null pointer");
    carve(nn_carve, P, workspace);
    P.pts = query; P.n = n_query; P.fp64 = fp64 ? 1 : 0;
    P.order = reinterpret_cast<const long long *>(qorder);
    P.dist = dist; P.idx = reinterpret_cast<long long *>(idx); P.ncand = ncand;
    NSR_LAUNCH(nsr::nn_query_kernel, dim3(nblk(n_query, 64)), dim3(64), 0, stream, P);
    return finish("nsr_nn_query");
}

int64_t nsr_sample_workspace_bytes(int64_t nf) {
    if (nf < 0) return -1;
    return pad16(8 * nf) + 8 * ((nf + nsr::kSurfTile - 1) / nsr::kSurfTile + 1);
}

int nsr_sample_surface(const double *verts, int64_t nv, const int32_t *faces, int64_t nf, int64_t n, const double *uniforms,
                       uint64_t seed, void *workspace, double *points, int64_t *face_index, void *stream) {
    if (nv < 0 || nf < 0 || n < 0) return fail("nsr_sample_surface: negative count");
    if (nv > 2147483647ll) return fail("nsr_sample_surface: more than 2^31 - 1 vertices");
    if (n == 0) return 0;
    if (nf == 0) return fail("nsr_sample_surface: the mesh has no faces");
    if (!verts || !faces || !workspace || !points || !face_index) return fail("nsr_sample_surface: null pointer");
    nsr::SurfSampleParams P;
    std::memset(&P, 0, sizeof(P));
    P.verts = verts; P.faces = faces; P.nv = nv; P.nf = nf; P.n = n;
    P.ntiles = (nf + nsr::kSurfTile - 1) / nsr::kSurfTile;
    P.cum = static_cast<double *>(workspace);
    P.tile = reinterpret_cast<double *>(static_cast<char *>(workspace) + pad16(8 * nf));
    P.uniforms = uniforms; P.seed = seed; P.points = points; P.face_index = reinterpret_cast<long long *>(face_index);
    NSR_LAUNCH(nsr::surf_tile_kernel, dim3(nblk(P.ntiles, 64)), dim3(64), 0, stream, P);
    NSR_LAUNCH(nsr::surf_tile_scan_kernel, dim3(1), dim3(64), 0, stream, P);
    NSR_LAUNCH(nsr::surf_cum_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::surf_point_kernel, dim3(nblk(n, 256)), dim3(256), 0, stream, P);
    return finish("nsr_sample_surface");
}

int64_t nsr_recon_partial_doubles(int64_t n) {
    if (n < 0) return -1;
    return 9 * ((n + nsr::kRedThreads - 1) / nsr::kRedThreads + 1);
}

int nsr_dist_stats(const double *dist, int64_t n, double th, double *partial, double *out, void *stream) {
    if (n < 0) return fail("nsr_dist_stats: negative count");
    if (!partial || !out || (n > 0 && !dist)) return fail("nsr_dist_stats: null pointer");
    nsr::RedParams P;
    std::memset(&P, 0, sizeof(P));
    P.dist = dist; P.n = n; P.th = th; P.partial = partial; P.out = out;
    P.nblocks = (n + nsr::kRedThreads - 1) / nsr::kRedThreads;
    if (P.nblocks > 0)
        NSR_LAUNCH(nsr::reduce_kernel<nsr::kRedDist>, dim3((unsigned)P.nblocks), dim3(nsr::kRedThreads), 2 * nsr::kRedThreads * 8, stream, P);
    NSR_LAUNCH(nsr::reduce_final_kernel<nsr::kRedDist>, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_dist_stats");
}

int nsr_icp_stats(const double *src, const double *tgt, const int64_t *idx, const double *dist, int64_t n, int64_t n_tgt, double th,
                  double *partial, double *out, void *stream) {
    if (n < 0 || n_tgt < 0) return fail("nsr_icp_stats: negative count");
    if (!partial || !out || (n > 0 && (!src || !tgt || !idx || !dist))) return fail("nsr_icp_stats: null pointer");
    nsr::RedParams P;
    std::memset(&P, 0, sizeof(P));
    P.src = src; P.tgt = tgt; P.idx = reinterpret_cast<const long long *>(idx); P.dist = dist; P.n = n; P.m = n_tgt; P.th = th;
    P.partial = partial; P.out = out;
    P.nblocks = (n + nsr::kRedThreads - 1) / nsr::kRedThreads;
    if (P.nblocks > 0)
        NSR_LAUNCH(nsr::reduce_kernel<nsr::kRedIcp1>, dim3((unsigned)P.nblocks), dim3(nsr::kRedThreads), 8 * nsr::kRedThreads * 8, stream, P);
    NSR_LAUNCH(nsr::reduce_final_kernel<nsr::kRedIcp1>, dim3(1), dim3(64), 0, stream, P);
    if (P.nblocks > 0)
        NSR_LAUNCH(nsr::reduce_kernel<nsr::kRedIcp2>, dim3((unsigned)P.nblocks), dim3(nsr::kRedThreads), 9 * nsr::kRedThreads * 8, stream, P);
    NSR_LAUNCH(nsr::reduce_final_kernel<nsr::kRedIcp2>, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_icp_stats");
}

int nsr_transform_points(double *pts, int64_t n, const double *m, void *stream) {
    if (n < 0) return fail("nsr_transform_points: negative count");
    if (n == 0) return 0;
    if (!pts || !m) return fail("nsr_transform_points: null pointer");
    nsr::XformParams P;
    P.pts = pts; P.n = n;
    for (int k = 0; k < 12; ++k) P.m[k] = m[k];
    NSR_LAUNCH(nsr::transform_points_kernel, dim3(nblk(n, 256)), dim3(256), 0, stream, P);
    return finish("nsr_transform_points");
}

int nsr_cull_vertices(const void *verts, int64_t n, int32_t fp64, const float *w2c, int32_t K, int32_t H, int32_t W, double fx,
                      double fy, double cx, double cy, const int32_t *faces, int64_t nf, uint8_t *seen, uint8_t *keep, void *stream) {
    if (n < 0 || nf < 0 || K < 0) return fail("nsr_cull_vertices: negative count");
    if (n > 2147483647ll) return fail("nsr_cull_vertices: more than 2^31 - 1 vertices");
    if (H < 1 || W < 1) return fail("nsr_cull_vertices: empty image");
    if ((n > 0 && (!verts || !seen || (K > 0 && !w2c))) || (nf > 0 && (!faces || !keep))) return fail("nsr_cull_vertices: null pointer");
    nsr::CullParams P;
    std::memset(&P, 0, sizeof(P));
    P.verts = verts; P.n = n; P.nf = nf; P.fp64 = fp64 ? 1 : 0; P.K = K; P.w2c = w2c;
    const double km[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) P.kf[i] = (float)km[i];
    P.W = (float)W; P.H = (float)H; P.faces = faces; P.seen = seen; P.keep = keep;
    if (n > 0) NSR_LAUNCH(nsr::cull_vertex_kernel, dim3(nblk(n, nsr::kCullThreads)), dim3(nsr::kCullThreads), nsr::kCullChunk * 12 * 4, stream, P);
    if (nf > 0) NSR_LAUNCH(nsr::cull_face_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    return finish("nsr_cull_vertices");
}

}  // extern "C"

// ---- point-to-mesh distance (include/nsr.h, "Point-to-mesh distance") ----
namespace {

// workspace of nsr_meshdist_build / nsr_meshdist_query
void md_carve(nsr::MdParams &P, Carve &c) {
    P.tri = c.take<double>(9 * P.nf);
    P.pface = c.take<int>(P.npairs);
    P.olist = c.take<int>(P.nover);
    carve_runs(c, P.G);
    P.crep = c.take<double>(3 * P.G.ncoarse);
}

// the mesh and its grid as MdParams; false with the error set
bool md_setup(nsr::MdParams &P, const char *who, const double *plan, const void *verts, int64_t nv, int32_t fp64, const int32_t *faces,
              int64_t nf) {
    std::memset(&P, 0, sizeof(P));
    if (nf < 1) { fail(std::string(who) + ": the mesh has no faces"); return false; }
    if (nv < 1 || nv > 2147483647ll || nf > 2147483647ll / 3) { fail(std::string(who) + ": vertex or face count outside int32 indexing"); return false; }
    if (!grid_from_plan(P.G, plan, nf)) { fail(std::string(who) + ": invalid plan for this mesh"); return false; }
    P.verts = verts; P.nv = nv; P.vfp64 = fp64 ? 1 : 0; P.faces = faces; P.nf = nf;
    return true;
}

bool md_counts_ok(const char *who, int64_t nf, int64_t npairs, int64_t nover) {
    if (npairs < 0 || nover < 0 || nover > nf || npairs > (int64_t)nsr::kMdCellCap * nf) { fail(std::string(who) + ": pair or oversize count outside the mesh's range"); return false; }
    if (npairs >= 2147483647ll) { fail(std::string(who) + ": the pair table overflows int32 indexing"); return false; }
    return true;
}

}  // namespace

extern "C" {

int nsr_meshdist_plan(const double *bounds, int64_t nf, double *plan) {
    if (nf < 1) return fail("nsr_meshdist_plan: the mesh has no faces");
    if (nf > 2147483647ll / 3) return fail("nsr_meshdist_plan: more faces than int32 indexing holds");
    if (nsr_nn_plan(bounds, nf, plan) != 0) return fail("nsr_meshdist_plan: no grid for these bounds (" + g_err + ")");
    return 0;
}

int64_t nsr_meshdist_workspace_bytes(const double *plan, int64_t nf, int64_t n_pairs, int64_t n_over) {
    nsr::MdParams P;
    std::memset(&P, 0, sizeof(P));
    if (nf < 1 || !grid_from_plan(P.G, plan, nf) || !md_counts_ok("nsr_meshdist_workspace_bytes", nf, n_pairs, n_over)) return -1;
    P.nf = nf; P.npairs = n_pairs; P.nover = n_over;
    return carve(md_carve, P);
}

int nsr_meshdist_count(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan, int64_t *count,
                       int64_t *over, void *stream) {
    nsr::MdParams P;
    if (!md_setup(P, "nsr_meshdist_count", plan, verts, nv, fp64, faces, nf)) return 1;
    if (!verts || !faces || !count || !over) return fail("nsr_meshdist_count: null pointer");
    P.count = reinterpret_cast<long long *>(count); P.over = reinterpret_cast<long long *>(over);
    NSR_LAUNCH(nsr::md_count_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    return finish("nsr_meshdist_count");
}

int nsr_meshdist_fill(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan,
                      const int64_t *count_cum, int64_t n_pairs, int64_t *keys, int64_t *pair_face, void *stream) {
    nsr::MdParams P;
    if (!md_setup(P, "nsr_meshdist_fill", plan, verts, nv, fp64, faces, nf)) return 1;
    if (!md_counts_ok("nsr_meshdist_fill", nf, n_pairs, 0)) return 1;
    if (n_pairs == 0) return 0;
    if (!verts || !faces || !count_cum || !keys || !pair_face) return fail("nsr_meshdist_fill: null pointer");
    P.cum = reinterpret_cast<const long long *>(count_cum); P.npairs = n_pairs;
    P.keys = reinterpret_cast<long long *>(keys); P.pair_face = reinterpret_cast<long long *>(pair_face);
    NSR_LAUNCH(nsr::md_fill_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    return finish("nsr_meshdist_fill");
}

int nsr_meshdist_build(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan,
                       const int64_t *sorted_keys, const int64_t *order, const int64_t *pair_face, int64_t n_pairs, const int64_t *over,
                       const int64_t *over_cum, int64_t n_over, void *workspace, void *stream) {
    nsr::MdParams P;
    if (!md_setup(P, "nsr_meshdist_build", plan, verts, nv, fp64, faces, nf)) return 1;
    if (!md_counts_ok("nsr_meshdist_build", nf, n_pairs, n_over)) return 1;
    if (!verts || !faces || !over || !over_cum || !workspace || (n_pairs > 0 && (!sorted_keys || !order || !pair_face)))
        return fail("nsr_meshdist_build: null pointer");
    P.npairs = n_pairs; P.nover = n_over;
    carve(md_carve, P, workspace);
    P.skeys = reinterpret_cast<const long long *>(sorted_keys); P.order = reinterpret_cast<const long long *>(order);
    P.pairs = reinterpret_cast<const long long *>(pair_face);
    P.over = const_cast<long long *>(reinterpret_cast<const long long *>(over)); P.ocum = reinterpret_cast<const long long *>(over_cum);
    const long long nclear = P.G.ncell > P.G.ncoarse ? P.G.ncell : P.G.ncoarse;
    NSR_LAUNCH(nsr::nn_clear_kernel, dim3(nblk(nclear, 256)), dim3(256), 0, stream, P.G);
    NSR_LAUNCH(nsr::md_tri_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    if (n_pairs > 0) NSR_LAUNCH(nsr::md_gather_kernel, dim3(nblk(n_pairs, 256)), dim3(256), 0, stream, P);
    return finish("nsr_meshdist_build");
}

int nsr_meshdist_query(const void *query, int64_t n_query, int32_t fp64, const int64_t *qorder, const double *plan, const void *workspace,
                       int64_t nf, int64_t n_pairs, int64_t n_over, double *dist, int64_t *face, double *closest, int32_t *ncand,
                       void *stream) {
    nsr::MdParams P;
    std::memset(&P, 0, sizeof(P));
    if (n_query < 0) return fail("nsr_meshdist_query: negative count");
    if (nf < 1 || !grid_from_plan(P.G, plan, nf)) return fail("nsr_meshdist_query: invalid plan for this mesh");
    if (!md_counts_ok("nsr_meshdist_query", nf, n_pairs, n_over)) return 1;
    if (n_query == 0) return 0;
    if (!query || !workspace || !dist || !face || !closest) return fail("nsr_meshdist_query: null pointer");
    P.nf = nf; P.npairs = n_pairs; P.nover = n_over;
    carve(md_carve, P, workspace);
    P.q = query; P.n = n_query; P.qfp64 = fp64 ? 1 : 0; P.qorder = reinterpret_cast<const long long *>(qorder);
    P.dist = dist; P.face = reinterpret_cast<long long *>(face); P.closest = closest; P.ncand = ncand;
    NSR_LAUNCH(nsr::md_query_kernel, dim3(nblk(n_query, 64)), dim3(64), 0, stream, P);
    return finish("nsr_meshdist_query");
}

int nsr_face_normals(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, double *normals, void *stream) {
    if (nv < 0 || nf < 0) return fail("nsr_face_normals: negative count");
    if (nv > 2147483647ll) return fail("nsr_face_normals: more than 2^31 - 1 vertices");
    if (nf == 0) return 0;
    if (!verts || !faces || !normals) return fail("nsr_face_normals: null pointer");
    nsr::MdNormalParams P;
    std::memset(&P, 0, sizeof(P));
    P.verts = verts; P.faces = faces; P.nv = nv; P.nf = nf; P.vfp64 = fp64 ? 1 : 0; P.normals = normals;
    NSR_LAUNCH(nsr::md_normals_kernel, dim3(nblk(nf, 256)), dim3(256), 0, stream, P);
    return finish("nsr_face_normals");
}

int nsr_normal_stats(const double *query_normals, const double *face_normals, const int64_t *face, int64_t n, int64_t nf, double *partial,
                     double *out, void *stream) {
    if (n < 0 || nf < 0) return fail("nsr_normal_stats: negative count");
    if (!partial || !out || (n > 0 && (!query_normals || !face_normals || !face))) return fail("nsr_normal_stats: null pointer");
    nsr::RedParams P;
    std::memset(&P, 0, sizeof(P));
    P.src = query_normals; P.tgt = face_normals; P.idx = reinterpret_cast<const long long *>(face); P.n = n; P.m = nf;
    P.partial = partial; P.out = out;
    P.nblocks = (n + nsr::kRedThreads - 1) / nsr::kRedThreads;
    if (P.nblocks > 0)
        NSR_LAUNCH(nsr::reduce_kernel<nsr::kRedNormal>, dim3((unsigned)P.nblocks), dim3(nsr::kRedThreads), 2 * nsr::kRedThreads * 8, stream, P);
    NSR_LAUNCH(nsr::reduce_final_kernel<nsr::kRedDist>, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_normal_stats");
}

}  // extern "C"

// ---- mesh bound from keyframes (include/nsr.h, "Mesh bound from keyframes") ----
namespace {

constexpr long long kTsdfMaxBits = 1ll << 31;        // dense unit bitmap: at most 2^31 units (256 MB)

int tsdf_setup(nsr::TsdfParams &P, const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, const float *w2c, double fx,
               double fy, double cx, double cy, double voxel_length, double sdf_trunc, const char *what) {
    std::memset(&P, 0, sizeof(P));
    if (K < 1 || H < 1 || W < 1) return fail(std::string(what) + ": need at least one frame of at least 1 x 1 pixels");
    if (!(voxel_length > 0.0) || !(sdf_trunc > 0.0) || !std::isfinite(voxel_length) || !std::isfinite(sdf_trunc))
        return fail(std::string(what) + ": voxel_length and sdf_trunc must be positive");
    if (!(fx != 0.0) || !(fy != 0.0)) return fail(std::string(what) + ": zero focal length");
    P.depth = depth; P.K = K; P.H = H; P.W = W; P.c2w = c2w; P.w2c = w2c;
    P.su = (W + nsr::kTsdfStride - 1) / nsr::kTsdfStride; P.sv = (H + nsr::kTsdfStride - 1) / nsr::kTsdfStride;
    P.npts = (long long)K * P.su * P.sv;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.vl = voxel_length; P.ul = voxel_length * nsr::kTsdfUnit; P.trunc = sdf_trunc;
    P.fxf = (float)fx; P.fyf = (float)fy; P.cxf = (float)cx; P.cyf = (float)cy; P.truncf = (float)sdf_trunc;
    P.tw = (K + 31) / 32;
    return 0;
}

// the bitmap layout for a HOST copy of the unit box; false if the box is empty or too large
bool tsdf_box(nsr::TsdfParams &P, const int32_t *box) {
    if (!box) return false;
    long long bits = 1;
    for (int d = 0; d < 3; ++d) {
        const long long n = (long long)box[3 + d] - box[d] + 1;
        if (n < 1 || n > (1 << 21)) return false;
        P.lo[d] = box[d];
        P.dim[d] = (int)n;
        bits *= n;
        if (bits > kTsdfMaxBits) return false;
    }
    P.nbits = bits;
    P.nwords = (bits + 31) / 32;
    P.nwblocks = (P.nwords + nsr::kBitsPerBlock - 1) / nsr::kBitsPerBlock;
    return true;
}

// workspace of the unit bitmap (tsdf_box's sizes)
void tsdf_carve(nsr::TsdfParams &P, Carve &c) {
    P.bitmap = c.take<unsigned>(P.nwords);
    P.wprefix = c.take<int>(P.nwords);
    P.bsum = c.take<long long>(P.nwblocks);
    P.nunits = c.take<long long>(1);
}

}  // namespace

extern "C" {

int nsr_tsdf_unit_box(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                      double voxel_length, double sdf_trunc, int32_t *box, void *stream) {
    nsr::TsdfParams P;
    if (int rc = tsdf_setup(P, depth, K, H, W, c2w, nullptr, fx, fy, cx, cy, voxel_length, sdf_trunc, "nsr_tsdf_unit_box")) return rc;
    if (!depth || !c2w || !box) return fail("nsr_tsdf_unit_box: null pointer");
    P.box = box;
    NSR_LAUNCH(nsr::tsdf_box_init_kernel, dim3(1), dim3(64), 0, stream, P);
    const long long nb = (P.npts + 255) / 256;
    NSR_LAUNCH(nsr::tsdf_box_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, stream, P);
    return finish("nsr_tsdf_unit_box");
}

int64_t nsr_tsdf_workspace_bytes(const int32_t *box) {
    nsr::TsdfParams P;
    std::memset(&P, 0, sizeof(P));
    if (!tsdf_box(P, box)) return -1;
    return carve(tsdf_carve, P);
}

int nsr_tsdf_touch_count(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                         double voxel_length, double sdf_trunc, const int32_t *box, void *workspace, int64_t *n_units, void *stream) {
    nsr::TsdfParams P;
    if (int rc = tsdf_setup(P, depth, K, H, W, c2w, nullptr, fx, fy, cx, cy, voxel_length, sdf_trunc, "nsr_tsdf_touch_count")) return rc;
    if (!tsdf_box(P, box)) return fail("nsr_tsdf_touch_count: empty unit box, or more than 2^31 units in it");
    if (!depth || !c2w || !workspace || !n_units) return fail("nsr_tsdf_touch_count: null pointer");
    carve(tsdf_carve, P, workspace);
    P.nunits = reinterpret_cast<long long *>(n_units);
    NSR_LAUNCH(nsr::tsdf_clear_kernel, dim3(nblk(P.nwords, 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::tsdf_mark_kernel, dim3(nblk(P.npts, 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::tsdf_wscan_kernel, dim3((unsigned)P.nwblocks), dim3(nsr::kBitsPerBlock), 4 * nsr::kBitsPerBlock, stream, P);
    NSR_LAUNCH(nsr::tsdf_bscan_kernel, dim3(1), dim3(64), 0, stream, P);
    NSR_LAUNCH(nsr::tsdf_wfix_kernel, dim3(nblk(P.nwords, 256)), dim3(256), 0, stream, P);
    return finish("nsr_tsdf_touch_count");
}

int nsr_tsdf_touch_emit(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                        double voxel_length, double sdf_trunc, const int32_t *box, const void *workspace, int64_t n_units, int32_t *units,
                        uint32_t *touch, void *stream) {
    nsr::TsdfParams P;
    if (int rc = tsdf_setup(P, depth, K, H, W, c2w, nullptr, fx, fy, cx, cy, voxel_length, sdf_trunc, "nsr_tsdf_touch_emit")) return rc;
    if (!tsdf_box(P, box)) return fail("nsr_tsdf_touch_emit: empty unit box, or more than 2^31 units in it");
    if (n_units < 0 || n_units > P.nbits) return fail("nsr_tsdf_touch_emit: unit count out of range");
    if (n_units == 0) return 0;
    if (!depth || !c2w || !workspace || !units || !touch) return fail("nsr_tsdf_touch_emit: null pointer");
    carve(tsdf_carve, P, workspace);
    P.n_units = n_units; P.units = units; P.touch = touch;
    NSR_LAUNCH(nsr::tsdf_units_kernel, dim3(nblk(P.nwords, 256)), dim3(256), 0, stream, P);
    NSR_LAUNCH(nsr::tsdf_touch_kernel, dim3(nblk(P.npts, 256)), dim3(256), 0, stream, P);
    return finish("nsr_tsdf_touch_emit");
}

int nsr_tsdf_integrate(const float *depth, int32_t K, int32_t H, int32_t W, const float *w2c, double fx, double fy, double cx, double cy,
                       double voxel_length, double sdf_trunc, const int32_t *units, const uint32_t *touch, int64_t n_units, float *tsdf,
                       float *weight, void *stream) {
    nsr::TsdfParams P;
    if (int rc = tsdf_setup(P, depth, K, H, W, nullptr, w2c, fx, fy, cx, cy, voxel_length, sdf_trunc, "nsr_tsdf_integrate")) return rc;
    if (n_units < 0 || n_units > 2147483647ll) return fail("nsr_tsdf_integrate: unit count out of range");
    if (n_units == 0) return 0;
    if (!depth || !w2c || !units || !touch || !tsdf || !weight) return fail("nsr_tsdf_integrate: null pointer");
    P.units = const_cast<int *>(units); P.touch = const_cast<unsigned *>(touch); P.n_units = n_units; P.tsdf = tsdf; P.weight = weight;
    NSR_LAUNCH(nsr::tsdf_integrate_kernel, dim3((unsigned)n_units), dim3(nsr::kTsdfThreads), 0, stream, P);
    return finish("nsr_tsdf_integrate");
}

int nsr_tsdf_surface_count(const int32_t *box, const void *workspace, const int32_t *units, int64_t n_units, const float *tsdf,
                           const float *weight, int64_t *counts, void *stream) {
    nsr::TsdfParams P;
    std::memset(&P, 0, sizeof(P));
    if (!tsdf_box(P, box)) return fail("nsr_tsdf_surface_count: empty unit box, or more than 2^31 units in it");
    if (n_units < 0 || n_units > P.nbits) return fail("nsr_tsdf_surface_count: unit count out of range");
    if (!counts) return fail("nsr_tsdf_surface_count: null pointer");
    if (n_units > 0 && (!workspace || !units || !tsdf || !weight)) return fail("nsr_tsdf_surface_count: null pointer");
    carve(tsdf_carve, P, workspace);
    P.units = const_cast<int *>(units); P.n_units = n_units;
    P.tsdf = const_cast<float *>(tsdf); P.weight = const_cast<float *>(weight); P.counts = reinterpret_cast<long long *>(counts);
    if (n_units > 0)
        NSR_LAUNCH(nsr::tsdf_surface_kernel<false>, dim3((unsigned)n_units), dim3(nsr::kTsdfThreads), 4 * (nsr::kTsdfThreads + 1), stream, P);
    NSR_LAUNCH(nsr::tsdf_count_scan_kernel, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_tsdf_surface_count");
}

int nsr_tsdf_surface_emit(const int32_t *box, const void *workspace, const int32_t *units, int64_t n_units, const float *tsdf,
                          const float *weight, double voxel_length, const int64_t *counts, int64_t n_points, double *points, void *stream) {
    nsr::TsdfParams P;
    std::memset(&P, 0, sizeof(P));
    if (!tsdf_box(P, box)) return fail("nsr_tsdf_surface_emit: empty unit box, or more than 2^31 units in it");
    if (n_units < 0 || n_units > P.nbits || n_points < 0) return fail("nsr_tsdf_surface_emit: count out of range");
    if (!(voxel_length > 0.0) || !std::isfinite(voxel_length)) return fail("nsr_tsdf_surface_emit: voxel_length must be positive");
    if (n_points == 0 || n_units == 0) return 0;
    if (!workspace || !units || !tsdf || !weight || !counts || !points) return fail("nsr_tsdf_surface_emit: null pointer");
    carve(tsdf_carve, P, workspace);
    P.units = const_cast<int *>(units); P.n_units = n_units;
    P.tsdf = const_cast<float *>(tsdf); P.weight = const_cast<float *>(weight);
    P.counts = const_cast<long long *>(reinterpret_cast<const long long *>(counts)); P.points = points;
    P.vl = voxel_length; P.ul = voxel_length * nsr::kTsdfUnit;
    NSR_LAUNCH(nsr::tsdf_surface_kernel<true>, dim3((unsigned)n_units), dim3(nsr::kTsdfThreads), 4 * (nsr::kTsdfThreads + 1), stream, P);
    return finish("nsr_tsdf_surface_emit");
}

int64_t nsr_hull_partial_doubles(void) { return 2ll * nsr::kHullBlocks * nsr::kHullDirs; }

int nsr_hull_extremes(const double *pts, int64_t n, double *partial, int64_t *ext, void *stream) {
    if (n < 1) return fail("nsr_hull_extremes: no points");
    if (!pts || !partial || !ext) return fail("nsr_hull_extremes: null pointer");
    nsr::HullParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = pts; P.n = n; P.fp64 = 1; P.partial = partial; P.ext = reinterpret_cast<long long *>(ext);
    NSR_LAUNCH(nsr::hull_extreme_kernel, dim3(nsr::kHullBlocks), dim3(256), 256 * 16, stream, P);
    NSR_LAUNCH(nsr::hull_extreme_final_kernel, dim3(1), dim3(64), 0, stream, P);
    return finish("nsr_hull_extremes");
}

int nsr_hull_prefilter(const double *pts, int64_t n, const double *planes, int32_t n_planes, double margin, uint8_t *keep, void *stream) {
    if (n < 0 || n_planes < 0 || n_planes > nsr::kHullMaxPlanes) return fail("nsr_hull_prefilter: count out of range (at most 64 planes)");
    if (!(margin >= 0.0)) return fail("nsr_hull_prefilter: negative margin");
    if (n == 0) return 0;
    if (!pts || !keep || (n_planes > 0 && !planes)) return fail("nsr_hull_prefilter: null pointer");
    nsr::HullParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = pts; P.n = n; P.fp64 = 1; P.n_planes = n_planes; P.margin = margin; P.out = keep;
    for (int j = 0; j < n_planes; ++j)
        for (int e = 0; e < 4; ++e) P.planes[j][e] = planes[4 * j + e];
    NSR_LAUNCH(nsr::hull_prefilter_kernel, dim3(nblk(n, 256)), dim3(256), 0, stream, P);
    return finish("nsr_hull_prefilter");
}

int nsr_convex_hull(const double *pts, int64_t n, double tol, double bound_scale, int64_t *counts, double *verts, int64_t *vert_index,
                    int32_t *faces, double *planes) {
    if (n < 0 || n > 2147483647ll) return fail("nsr_convex_hull: point count out of range");
    if (!(tol >= 0.0) || !(bound_scale > 0.0) || !std::isfinite(bound_scale)) return fail("nsr_convex_hull: tol must be >= 0, bound_scale > 0");
    if (!pts || !counts || !verts || !vert_index || !faces || !planes) return fail("nsr_convex_hull: null pointer");
    for (long long i = 0; i < 3 * n; ++i)
        if (!std::isfinite(pts[i])) return fail("nsr_convex_hull: non-finite coordinates");
    std::vector<nsr::HullFace> F;
    const int rc = nsr::hull_build(pts, n, tol, F);
    if (rc == -1) return fail("nsr_convex_hull: the points span no volume (fewer than 4, or all within tol of a plane)");
    if (rc != 0) return fail("nsr_convex_hull: the hull surface did not close (numerical breakdown)");
    std::vector<int> remap((size_t)n, -1);
    for (const auto &f : F)
        if (f.alive)
            for (int e = 0; e < 3; ++e) remap[f.v[e]] = 0;
    long long nv = 0, nf = 0;
    for (long long i = 0; i < n; ++i)
        if (remap[i] == 0) { remap[i] = (int)nv; vert_index[nv] = i; ++nv; }
    double c[3] = {0.0, 0.0, 0.0};
    for (long long v = 0; v < nv; ++v)
        for (int d = 0; d < 3; ++d) c[d] += pts[3 * vert_index[v] + d];
    for (int d = 0; d < 3; ++d) c[d] /= (double)nv;
    for (long long v = 0; v < nv; ++v)
        for (int d = 0; d < 3; ++d) verts[3 * v + d] = (pts[3 * vert_index[v] + d] - c[d]) * bound_scale + c[d];
    for (const auto &f : F) {
        if (!f.alive) continue;
        nsr::HullFace g;
        for (int e = 0; e < 3; ++e) { faces[3 * nf + e] = remap[f.v[e]]; g.v[e] = remap[f.v[e]]; }
        nsr::hull_plane(verts, g);
        for (int e = 0; e < 3; ++e) planes[4 * nf + e] = g.n[e];
        planes[4 * nf + 3] = g.off;
        ++nf;
    }
    counts[0] = nv; counts[1] = nf;
    return 0;
}

int nsr_hull_contains(const void *pts, int64_t n, int32_t fp64, const double *planes, int32_t n_planes, uint8_t *inside, void *stream) {
    if (n < 0 || n_planes < 0) return fail("nsr_hull_contains: negative count");
    if (n == 0) return 0;
    if (!pts || !inside || (n_planes > 0 && !planes)) return fail("nsr_hull_contains: null pointer");
    nsr::HullParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = pts; P.n = n; P.fp64 = fp64 ? 1 : 0; P.dplanes = planes; P.n_planes = n_planes; P.out = inside;
    NSR_LAUNCH(nsr::hull_contains_kernel, dim3(nblk(n, 256)), dim3(256), nsr::kContainsChunk * 4 * 8, stream, P);
    return finish("nsr_hull_contains");
}

}  // extern "C"

// ---- depth rasterization and the 2-D depth metric (include/nsr.h, "Depth rasterization") ----
namespace {

bool raster_sizes(nsr::RasterParams &P, int64_t nv, int64_t nf, int32_t K, int32_t H, int32_t W) {
    if (nv < 1 || nf < 1 || K < 1 || H < 1 || W < 1 || H > nsr::kRasterMaxTiles || W > nsr::kRasterMaxTiles) return false;
    if (nv > 2147483647ll || nf > 2147483647ll) return false;
    P.nv = nv; P.nf = nf; P.K = K; P.H = H; P.W = W;
    P.tx = (W + nsr::kRasterTile - 1) / nsr::kRasterTile;
    P.ty = (H + nsr::kRasterTile - 1) / nsr::kRasterTile;
    P.ntiles = P.tx * P.ty;
    P.nchunks = (nf + nsr::kRasterChunk - 1) / nsr::kRasterChunk;
    return true;
}

// workspace of nsr_raster_bin, read by nsr_raster_depth and nsr_view_mesh (raster_sizes' sizes)
void raster_carve(nsr::RasterParams &P, Carve &c) {
    P.cam = c.take<float>(4ll * P.K * P.nv);
    P.rect = c.take<int>(2ll * P.K * P.nf);
    P.counts = c.take<int>((long long)P.K * P.ntiles * P.nchunks);
    P.tile_start = c.take<long long>((long long)P.K * P.ntiles + 1);
}

int raster_setup(nsr::RasterParams &P, const float *verts, int64_t nv, const int32_t *faces, int64_t nf, const float *w2c, int32_t K,
                 int32_t H, int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace,
                 const char *what) {
    std::memset(&P, 0, sizeof(P));
    if (nv < 1 || nf < 1) return fail(std::string(what) + ": empty mesh");
    if (K < 1) return fail(std::string(what) + ": no views");
    if (!raster_sizes(P, nv, nf, K, H, W)) return fail(std::string(what) + ": image sizes must be 1..1024, at most 2^31 - 1 vertices and faces");
    if (!(near > 0.0) || !(far > near) || !std::isfinite(far) || far > 1e30) return fail(std::string(what) + ": need 0 < near < far (finite)");
    if (!(fx != 0.0) || !(fy != 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(std::string(what) + ": focal lengths must be finite and non-zero");
    if (!verts || !faces || !w2c || !workspace) return fail(std::string(what) + ": null pointer");
    P.verts = verts; P.faces = faces; P.w2c = w2c;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.near = near; P.far = far;
    P.fxf = (float)fx; P.fyf = (float)fy; P.cxf = (float)cx; P.cyf = (float)cy; P.nearf = (float)near; P.farf = (float)far;
    carve(raster_carve, P, workspace);
    return 0;
}

// partial sums per view of nsr_depth_error: one per block of pixels
long long depth_error_blocks(long long n_pixels) { return (n_pixels + nsr::kRasterThreads - 1) / nsr::kRasterThreads; }

}  // namespace

extern "C" {

int64_t nsr_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t H, int32_t W) {
    nsr::RasterParams P;
    std::memset(&P, 0, sizeof(P));
    if (!raster_sizes(P, n_verts, n_faces, K, H, W)) return -1;
    return carve(raster_carve, P);
}

int nsr_raster_bin(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                   int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int64_t *n_entries,
                   void *stream) {
    nsr::RasterParams P;
    if (int rc = raster_setup(P, verts, n_verts, faces, n_faces, w2c, K, H, W, fx, fy, cx, cy, near, far, workspace, "nsr_raster_bin")) return rc;
    if (!n_entries) return fail("nsr_raster_bin: null pointer");
    P.n_entries = reinterpret_cast<long long *>(n_entries);
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::raster_vertex_kernel, dim3(nblk(P.nv, T), K), dim3(T), 0, stream, P);
    NSR_LAUNCH(nsr::raster_setup_kernel, dim3(nblk(P.nf, T), K), dim3(T), 0, stream, P);
    NSR_LAUNCH(nsr::raster_count_kernel, dim3((unsigned)P.nchunks, K), dim3(T), 4 * 4 * P.ntiles, stream, P);
    NSR_LAUNCH(nsr::raster_scan_tile_kernel, dim3(P.ntiles, K), dim3(T), 2 * 4 * T, stream, P);
    NSR_LAUNCH(nsr::raster_scan_view_kernel, dim3(1), dim3(T), 8 * T, stream, P);
    return finish("nsr_raster_bin");
}

int nsr_raster_depth(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                     int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int32_t *bins,
                     int64_t n_entries, float *depth, void *stream) {
    nsr::RasterParams P;
    if (int rc = raster_setup(P, verts, n_verts, faces, n_faces, w2c, K, H, W, fx, fy, cx, cy, near, far, workspace, "nsr_raster_depth")) return rc;
    if (n_entries < 0) return fail("nsr_raster_depth: negative entry count");
    if (!depth || (n_entries > 0 && !bins)) return fail("nsr_raster_depth: null pointer");
    P.bins = bins; P.depth = depth; P.cap = n_entries;
    const int T = nsr::kRasterThreads;
    // (n_entries is what nsr_raster_bin counted into the same workspace: the emit writes exactly that many)
    if (n_entries > 0) NSR_LAUNCH(nsr::raster_emit_kernel, dim3((unsigned)P.nchunks, K), dim3(T), 4 * 4 * P.ntiles, stream, P);
    NSR_LAUNCH(nsr::raster_resolve_kernel, dim3(P.ntiles, K), dim3(T), nsr::kRasterResolveLds, stream, P);
    return finish("nsr_raster_depth");
}

int64_t nsr_depth_error_partial_doubles(int32_t K, int64_t n_pixels) {
    if (K < 1 || n_pixels < 1) return -1;
    return (long long)K * depth_error_blocks(n_pixels);
}

int nsr_depth_error(const float *a, const float *b, int32_t K, int64_t n_pixels, double *partial, double *out, void *stream) {
    if (K < 1 || n_pixels < 1) return fail("nsr_depth_error: need at least one view of at least one pixel");
    if (!a || !b || !partial || !out) return fail("nsr_depth_error: null pointer");
    nsr::L1Params P;
    std::memset(&P, 0, sizeof(P));
    P.a = a; P.b = b; P.n = n_pixels; P.K = K; P.partial = partial; P.out = out;
    P.nblocks = depth_error_blocks(n_pixels);
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::raster_l1_kernel, dim3((unsigned)P.nblocks, K), dim3(T), 8 * T, stream, P);
    NSR_LAUNCH(nsr::raster_l1_final_kernel, dim3(nblk(K, T)), dim3(T), 0, stream, P);
    return finish("nsr_depth_error");
}

int nsr_view_unseen(const void *pts, int64_t n, int32_t fp64, const float *w2c, int32_t K, int32_t H, int32_t W, double fx, double fy,
                    double cx, double cy, uint8_t *sees, void *stream) {
    if (n < 0 || K < 1) return fail("nsr_view_unseen: need at least one candidate and a non-negative point count");
    if (n > 2147483647ll) return fail("nsr_view_unseen: more than 2^31 - 1 points");
    if (H < 1 || W < 1) return fail("nsr_view_unseen: empty image");
    if (!w2c || !sees || (n > 0 && !pts)) return fail("nsr_view_unseen: null pointer");
    nsr::ViewParams V;
    std::memset(&V, 0, sizeof(V));
    V.C.verts = pts; V.C.n = n; V.C.fp64 = fp64 ? 1 : 0; V.C.K = K; V.C.w2c = w2c;
    const double km[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) V.C.kf[i] = (float)km[i];
    V.C.W = (float)W; V.C.H = (float)H; V.sees = sees;
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::raster_view_clear_kernel, dim3(nblk(K, T)), dim3(T), 0, stream, V);
    if (n > 0) NSR_LAUNCH(nsr::raster_view_kernel, dim3(nblk(n, T)), dim3(T), nsr::kRasterViewChunk * 12 * 4, stream, V);
    return finish("nsr_view_unseen");
}

int nsr_points_visible(const void *pts, int64_t n, int32_t fp64, const float *w2c, int32_t K, const float *depth, int32_t H, int32_t W,
                       double fx, double fy, double cx, double cy, double near, double far, double eps, int32_t *count, void *stream) {
    if (n < 1) return fail("nsr_points_visible: no points");
    if (n > 2147483647ll) return fail("nsr_points_visible: more than 2^31 - 1 points");
    if (K < 1) return fail("nsr_points_visible: no views");
    if (H < 1 || W < 1) return fail("nsr_points_visible: empty image");
    if (!(near < far)) return fail("nsr_points_visible: need near < far");
    if (!(eps >= 0.0)) return fail("nsr_points_visible: eps must be non-negative");
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("nsr_points_visible: intrinsics must be finite");
    if (!pts || !w2c || !depth || !count) return fail("nsr_points_visible: null pointer");
    nsr::VisParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = pts; P.n = n; P.fp64 = fp64 ? 1 : 0; P.K = K; P.H = H; P.W = W; P.w2c = w2c; P.depth = depth;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.near = near; P.far = far; P.eps = eps; P.count = count;
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::points_visible_kernel, dim3(nblk(n, T)), dim3(T), nsr::kRasterViewChunk * 12 * 4, stream, P);
    return finish("nsr_points_visible");
}

}  // extern "C"

// ---- replay view: vertex normals, the shaded mesh layer and the point layer (include/nsr.h, "Replay view") ----
extern "C" {

int64_t nsr_view_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t H, int32_t W) {
    return nsr_raster_workspace_bytes(n_verts, n_faces, K, H, W);      // the mesh layer draws from nsr_raster_bin's workspace
}

int nsr_view_normals(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const int64_t *start,
                     const int32_t *incident, int64_t n_incident, double *sums, float *normals, void *stream) {
    if (n_verts < 1 || n_faces < 1) return fail("nsr_view_normals: empty mesh");
    if (n_verts > 2147483647ll || n_faces > 2147483647ll) return fail("nsr_view_normals: more than 2^31 - 1 vertices or faces");
    if (n_incident < 0 || n_incident > 3 * n_faces) return fail("nsr_view_normals: the incidence list holds 0 .. 3 n_faces entries");
    if (!verts || !faces || !start || !normals || (n_incident > 0 && !incident)) return fail("nsr_view_normals: null pointer");
    nsr::NormalParams P;
    std::memset(&P, 0, sizeof(P));
    P.verts = verts; P.faces = faces; P.nv = n_verts; P.nf = n_faces;
    P.start = reinterpret_cast<const long long *>(start); P.incident = incident; P.n_incident = n_incident;
    P.sums = sums; P.normals = normals;
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::view_normals_kernel, dim3(nblk(n_verts, T)), dim3(T), 0, stream, P);
    return finish("nsr_view_normals");
}

int nsr_view_mesh(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                  int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int32_t *bins,
                  int64_t n_entries, const float *normals, const uint8_t *colors, int32_t cull, float *depth, int32_t *face,
                  uint8_t *rgb, void *stream) {
    nsr::MeshViewParams M;
    std::memset(&M, 0, sizeof(M));
    nsr::RasterParams &P = M.R;
    if (int rc = raster_setup(P, verts, n_verts, faces, n_faces, w2c, K, H, W, fx, fy, cx, cy, near, far, workspace, "nsr_view_mesh")) return rc;
    if (cull != nsr::kViewCullNone && cull != nsr::kViewCullBack && cull != nsr::kViewCullFront)
        return fail("nsr_view_mesh: bad cull mode (NSR_CULL_NONE, NSR_CULL_BACK or NSR_CULL_FRONT)");
    if (n_entries < 0) return fail("nsr_view_mesh: negative entry count");
    if (!normals || !depth || !face || !rgb || (n_entries > 0 && !bins)) return fail("nsr_view_mesh: null pointer");
    P.bins = bins; P.depth = depth; P.cap = n_entries;
    M.normals = normals; M.colors = colors; M.cull = cull; M.face = face; M.rgb = rgb;
    const int T = nsr::kRasterThreads;
    if (n_entries > 0) NSR_LAUNCH(nsr::raster_emit_kernel, dim3((unsigned)P.nchunks, K), dim3(T), 4 * 4 * P.ntiles, stream, P);
    NSR_LAUNCH(nsr::view_resolve_kernel, dim3(P.ntiles, K), dim3(T), nsr::kViewResolveLds, stream, M);
    return finish("nsr_view_mesh");
}

int nsr_view_points(const float *pts, const uint8_t *colors, int64_t n, const int64_t *offsets, const float *w2c, int32_t B, int32_t H,
                    int32_t W, double fx, double fy, double cx, double cy, double near, double far, int32_t size,
                    const uint8_t *base_rgb, const float *base_depth, int32_t base_per_frame, uint8_t *rgb, int32_t *owner, void *stream) {
    if (B < 1) return fail("nsr_view_points: no views");
    if (B > 65535) return fail("nsr_view_points: more than 65535 frames in one call");
    if (H < 1 || W < 1 || H > nsr::kRasterMaxTiles || W > nsr::kRasterMaxTiles) return fail("nsr_view_points: image sizes must be 1..1024");
    if (n < 0 || n > 2147483647ll) return fail("nsr_view_points: 0 .. 2^31 - 1 points");
    if (size < 1 || size > nsr::kViewMaxPointSize) return fail("nsr_view_points: point size must be 1..64");
    if (!(near > 0.0) || !(far > near) || !std::isfinite(far)) return fail("nsr_view_points: need 0 < near < far (finite)");
    if (!(fx != 0.0) || !(fy != 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail("nsr_view_points: focal lengths must be finite and non-zero");
    if (!offsets || !w2c || !base_rgb || !base_depth || !rgb || (n > 0 && (!pts || !colors))) return fail("nsr_view_points: null pointer");
    nsr::PointViewParams P;
    std::memset(&P, 0, sizeof(P));
    P.pts = pts; P.colors = colors; P.offsets = reinterpret_cast<const long long *>(offsets); P.n = n; P.w2c = w2c;
    P.B = B; P.H = H; P.W = W; P.size = size; P.base_per_frame = base_per_frame ? 1 : 0;
    P.tx = (W + nsr::kRasterTile - 1) / nsr::kRasterTile;
    P.ty = (H + nsr::kRasterTile - 1) / nsr::kRasterTile;
    P.ntiles = P.tx * P.ty;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.near = near; P.far = far;
    P.base_rgb = base_rgb; P.base_depth = base_depth; P.rgb = rgb; P.owner = owner;
    const int T = nsr::kRasterThreads;
    NSR_LAUNCH(nsr::view_points_kernel, dim3(P.ntiles, B), dim3(T), 8 * nsr::kRasterTile * nsr::kRasterTile, stream, P);
    return finish("nsr_view_points");
}

}  // extern "C"

// ---- rendering evaluation (include/nsr.h, "Rendering evaluation") ----
namespace {

// tiles of window positions per row and per column; false: sizes the kernel does not take
bool imgmetrics_tiles(int32_t B, int32_t H, int32_t W, int &tx, int &ty) {
    if (B < 0 || B > 65535 || H < nsr::kImWin || W < nsr::kImWin || H > 32768 || W > 32768) return false;
    tx = (W - (nsr::kImWin - 1) + nsr::kImTile - 1) / nsr::kImTile;
    ty = (H - (nsr::kImWin - 1) + nsr::kImTile - 1) / nsr::kImTile;
    return true;
}

// the tiles' partial sums (doubles)
long long imgmetrics_bytes(int32_t B, int tx, int ty) { return 8ll * nsr::kImPartials * B * tx * ty; }

}  // namespace

extern "C" {

int64_t nsr_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    int tx = 0, ty = 0;
    if (!imgmetrics_tiles(B, H, W, tx, ty)) return -1;
    return imgmetrics_bytes(B, tx, ty);
}

int nsr_image_metrics(const float *color, const float *gt_color, const float *depth, const float *gt_depth, int32_t B, int32_t H, int32_t W,
                      double *result, float *depth_residual, float *color_residual, void *workspace, int64_t workspace_bytes, void *stream) {
    if (B < 0) return fail("nsr_image_metrics: negative batch size");
    if (H < nsr::kImWin || W < nsr::kImWin) return fail("nsr_image_metrics: images must be at least 11 x 11 (one SSIM window)");
    nsr::ImgMetricsParams P;
    std::memset(&P, 0, sizeof(P));
    if (!imgmetrics_tiles(B, H, W, P.tx, P.ty)) return fail("nsr_image_metrics: at most 65535 frames of at most 32768 x 32768");
    if (B == 0) return 0;
    if (!color || !gt_color || !depth || !gt_depth || !result || !workspace) return fail("nsr_image_metrics: null pointer");
    P.ntiles = P.tx * P.ty;
    if (workspace_bytes < imgmetrics_bytes(B, P.tx, P.ty))
        return fail("nsr_image_metrics: workspace too small (nsr_image_metrics_workspace_bytes)");
    P.color = color; P.gt_color = gt_color; P.depth = depth; P.gt_depth = gt_depth;
    P.B = B; P.H = H; P.W = W;
    P.partial = static_cast<double *>(workspace); P.out = result;
    P.depth_res = depth_residual; P.color_res = color_residual;
    double g[nsr::kImWin], sum = 0.0;
    for (int i = 0; i < nsr::kImWin; ++i) {
        const double d = i - nsr::kImWin / 2;
        g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < nsr::kImWin; ++i) P.g[i] = (float)(g[i] / sum);
    if (int rc = launch_cfg(nsr::imgmetrics_tile_kernel, nsr::kImLds, "nsr_image_metrics")) return rc;
    const int T = nsr::kImThreads;
    NSR_LAUNCH(nsr::imgmetrics_tile_kernel, dim3(P.ntiles, B), dim3(T), nsr::kImLds, stream, P);
    NSR_LAUNCH(nsr::imgmetrics_final_kernel, dim3(B), dim3(T), nsr::kImFinalLds, stream, P);
    return finish("nsr_image_metrics");
}

}  // extern "C"

// ---- rendering figures (include/nsr.h, "Rendering figures") ----
namespace {

constexpr int kFigMaxSide = 32768;

// nullptr: the sizes are valid and P's layout fields are filled; else what is wrong with them
const char *figure_geometry(int32_t H, int32_t W, int32_t stride, int32_t margin, int32_t gap, nsr::FigureParams &P) {
    if (H < 1 || W < 1 || H > kFigMaxSide || W > kFigMaxSide) return "image sizes must be in [1, 32768]";
    if (stride < 1 || stride > kFigMaxSide) return "stride must be in [1, 32768]";
    if (margin < 0 || gap < 0 || margin > kFigMaxSide || gap > kFigMaxSide) return "margin and gap must be in [0, 32768]";
    P.H = H; P.W = W; P.stride = stride; P.margin = margin; P.gap = gap;
    P.h = (H + stride - 1) / stride;
    P.w = (W + stride - 1) / stride;
    P.SH = 2 * margin + 2 * P.h + gap;
    P.SW = 2 * margin + 3 * P.w + 2 * gap;
    if (3ll * P.SH * P.SW >= (1ll << 31)) return "the sheet must stay below 2^31 bytes per frame";
    return nullptr;
}

// launches 1 and 2 of nsr_figure.h (the frames' maxima, into P.vmax_out or the slots), then 3 and, without a buffer, 4
int figure_launch(nsr::FigureParams &P, bool own_max, void *stream, const char *what) {
    const int T = nsr::kFigThreads;
    const long long frame_bytes = 3ll * P.SH * P.SW, groups = (P.npix + nsr::kFigLane - 1) / nsr::kFigLane;
    if (nblk(groups, T) > 2147483647ll) return fail(std::string(what) + ": too many pixels for one launch");
    if (reinterpret_cast<uintptr_t>(P.out) & 3) return fail(std::string(what) + ": the output must be 4-byte aligned");
    P.skip_slot = 0;
    if (own_max && !P.tiny) {
        long long np = ((long long)P.H * P.W + nsr::kFigMaxChunk - 1) / nsr::kFigMaxChunk;
        if (np > (frame_bytes - 8) / 4) np = (frame_bytes - 8) / 4;                 // slot + partials + 3 bytes of alignment fit the frame
        P.np = (int)np;
        NSR_LAUNCH(nsr::figure_max_partial_kernel, dim3(P.np, P.B), dim3(T), 4 * T, stream, P);
        NSR_LAUNCH(nsr::figure_max_final_kernel, dim3(P.B), dim3(T), 4 * T, stream, P);
        P.vmax = P.vmax_out;
        P.skip_slot = P.vmax_out ? 0 : 1;
    }
    NSR_LAUNCH(nsr::figure_sheet_kernel, dim3((unsigned)nblk(groups, T)), dim3(T), nsr::kFigLds, stream, P);
    if (P.skip_slot) NSR_LAUNCH(nsr::figure_slot_kernel, dim3((unsigned)nblk(P.B, T)), dim3(T), nsr::kFigLds, stream, P);
    return finish(what);
}

}  // namespace

extern "C" {

int nsr_figure_sheet_size(int32_t H, int32_t W, int32_t stride, int32_t margin, int32_t gap, int32_t *SH, int32_t *SW) {
    nsr::FigureParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = figure_geometry(H, W, stride, margin, gap, P)) return fail(std::string("nsr_figure_sheet_size: ") + e);
    if (!SH || !SW) return fail("nsr_figure_sheet_size: null pointer");
    *SH = P.SH;
    *SW = P.SW;
    return 0;
}

int nsr_figure_sheet(const float *color, const float *gt_color, const float *depth, const float *gt_depth, int32_t B, int32_t H, int32_t W,
                     int32_t stride, int32_t margin, int32_t gap, float *vmax_out, uint8_t *sheet, void *stream) {
    nsr::FigureParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = figure_geometry(H, W, stride, margin, gap, P)) return fail(std::string("nsr_figure_sheet: ") + e);
    if (B < 0 || B > 65535) return fail("nsr_figure_sheet: the batch size must be in [0, 65535]");
    if (B == 0) return 0;
    if (!color || !gt_color || !depth || !gt_depth || !sheet) return fail("nsr_figure_sheet: null pointer");
    P.color = color; P.gt_color = gt_color; P.depth = depth; P.gt_depth = gt_depth;
    P.vmax_out = vmax_out; P.out = sheet; P.B = B; P.sheet = 1;
    P.npix = (long long)B * P.SH * P.SW;
    return figure_launch(P, true, stream, "nsr_figure_sheet");
}

int nsr_depth_colorize(const float *depth, int32_t B, int32_t H, int32_t W, const float *vmax, uint8_t *rgb, void *stream) {
    nsr::FigureParams P;
    std::memset(&P, 0, sizeof(P));
    if (H < 1 || W < 1 || H > kFigMaxSide || W > kFigMaxSide) return fail("nsr_depth_colorize: image sizes must be in [1, 32768]");
    if (3ll * H * W >= (1ll << 31)) return fail("nsr_depth_colorize: the image must stay below 2^31 bytes");
    if (B < 0 || B > 65535) return fail("nsr_depth_colorize: the batch size must be in [0, 65535]");
    if (B == 0) return 0;
    if (!depth || !rgb) return fail("nsr_depth_colorize: null pointer");
    P.depth = depth; P.vmax = vmax; P.out = rgb; P.B = B; P.H = H; P.W = W; P.stride = 1; P.h = H; P.w = W; P.SH = H; P.SW = W;
    P.npix = (long long)B * H * W;
    P.tiny = !vmax && (long long)H * W < nsr::kFigTinyPixels ? 1 : 0;
    return figure_launch(P, vmax == nullptr, stream, "nsr_depth_colorize");
}

}  // extern "C"

// ---- JPEG encoding (include/nsr.h, "JPEG encoding") ----
namespace {

// nullptr: the sizes are valid, P's geometry is filled and out_bytes is the output's capacity; else what is wrong with them
const char *jpeg_geometry(int32_t n, int32_t H, int32_t W, int32_t subsampling, nsr::JpegParams &P, long long &out_bytes) {
    if (n < 0 || n > 65535) return "the batch size must be in [0, 65535]";
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return "image sizes must be in [1, 65535]";
    if (subsampling != 0 && subsampling != 2) return "subsampling must be 0 (4:4:4) or 2 (4:2:0)";
    P.n = n; P.H = H; P.W = W;
    P.sub = subsampling == 0 ? 1 : 2;
    const int side = 8 * P.sub;
    P.mcux = (W + side - 1) / side;
    P.mcuy = (H + side - 1) / side;
    P.bpm = P.sub == 1 ? 3 : 6;
    P.BI = P.mcux * P.bpm;
    const long long nint = (long long)n * P.mcuy;
    P.nblocks = nint * P.BI;
    if (nint > 2147483647ll || P.nblocks > 2147483647ll) return "too many blocks for one call";
    P.nint = (int)nint;
    const long long rawcap = ((long long)P.BI * nsr::kJpgBlockBits + 7) / 8;
    P.rawstride = (unsigned)pad16(rawcap);
    out_bytes = n * (P.mcuy * 2 * rawcap + 2ll * (P.mcuy - 1));
    return nullptr;
}

void jpeg_carve(nsr::JpegParams &P, Carve &c) {
    P.coef = c.take<short>(64 * P.nblocks);
    P.bitoff = c.take<unsigned>(P.nblocks);
    P.raw = c.take<unsigned char>((long long)P.nint * P.rawstride);
    P.ibits = c.take<unsigned>(P.nint);
    P.nff = c.take<unsigned>(P.nint);
    P.ioff = c.take<long long>(P.nint);
    P.ftot = c.take<long long>(P.n);
}

}  // namespace

extern "C" {

int nsr_jpeg_size(int32_t n, int32_t H, int32_t W, int32_t subsampling, int64_t *workspace_bytes, int64_t *out_bytes) {
    nsr::JpegParams P;
    long long cap = 0;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = jpeg_geometry(n, H, W, subsampling, P, cap)) return fail(std::string("nsr_jpeg_size: ") + e);
    if (!workspace_bytes || !out_bytes) return fail("nsr_jpeg_size: null pointer");
    *workspace_bytes = carve(jpeg_carve, P);
    *out_bytes = cap;
    return 0;
}

int nsr_jpeg_encode(const uint8_t *images, int32_t n, int32_t H, int32_t W, int32_t quality, int32_t subsampling, void *workspace,
                    int64_t workspace_bytes, uint8_t *out, int64_t out_bytes, int64_t *offsets, void *stream) {
    nsr::JpegParams P;
    long long cap = 0;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = jpeg_geometry(n, H, W, subsampling, P, cap)) return fail(std::string("nsr_jpeg_encode: ") + e);
    if (quality < 1 || quality > 100) return fail("nsr_jpeg_encode: quality must be in [1, 100]");
    if (n == 0) return 0;
    if (!images || !workspace || !out || !offsets) return fail("nsr_jpeg_encode: null pointer");
    if (workspace_bytes < carve(jpeg_carve, P, workspace) || out_bytes < cap) return fail("nsr_jpeg_encode: workspace or output smaller than nsr_jpeg_size reports");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail("nsr_jpeg_encode: the workspace must be 16-byte aligned");
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            const int v = (nsr::kJpgQuantBase[c][nsr::kJpgZigzag[k]] * scale + 50) / 100;
            P.q[c][k] = (unsigned char)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    P.img = images;
    P.out = out;
    P.offsets = reinterpret_cast<long long *>(offsets);
    const int T = nsr::kJpgThreads, scan_lds = nsr::kJpgScanLds;
    if (P.sub == 1) NSR_LAUNCH(nsr::jpeg_transform_kernel<1>, dim3(nblk(P.nblocks, T)), dim3(T), 0, stream, P);
    else NSR_LAUNCH(nsr::jpeg_transform_kernel<2>, dim3(nblk(P.nblocks, T)), dim3(T), 0, stream, P);
    NSR_LAUNCH(nsr::jpeg_measure_kernel, dim3(P.nint), dim3(T), nsr::kJpgMeasureLds, stream, P);
    NSR_LAUNCH(nsr::jpeg_pack_kernel, dim3(P.nint), dim3(T), nsr::kJpgPackLds, stream, P);
    NSR_LAUNCH(nsr::jpeg_count_kernel, dim3(P.nint), dim3(T), scan_lds, stream, P);
    NSR_LAUNCH(nsr::jpeg_offsets_kernel, dim3(P.n), dim3(T), scan_lds, stream, P, 0);
    NSR_LAUNCH(nsr::jpeg_offsets_kernel, dim3(1), dim3(T), scan_lds, stream, P, 1);
    NSR_LAUNCH(nsr::jpeg_stuff_kernel, dim3(P.nint), dim3(T), scan_lds, stream, P);
    return finish("nsr_jpeg_encode");
}

}  // extern "C"

// ---- JPEG decoding (include/nsr.h, "JPEG decoding") ----
namespace {

// nullptr: the sizes are valid and P's geometry is filled; else what is wrong with them
const char *jpegdec_geometry(int32_t n, int32_t H, int32_t W, int32_t sampling, int32_t subsequence_bytes, nsr::JpegDecParams &P) {
    if (n < 0 || n > 65535) return "the batch size must be in [0, 65535]";
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return "image sizes must be in [1, 65535]";
    if (sampling < NSR_JPEG_444 || sampling > NSR_JPEG_GREY) return "sampling must be 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) or 3 (one component)";
    if (subsequence_bytes < 16 || subsequence_bytes > 1024 || subsequence_bytes % 4) return "subsequence_bytes must be a multiple of 4 in [16, 1024]";
    P.n = n; P.H = H; P.W = W; P.sub_bytes = subsequence_bytes;
    P.hs = sampling == NSR_JPEG_422 || sampling == NSR_JPEG_420 ? 2 : 1;
    P.vs = sampling == NSR_JPEG_420 ? 2 : 1;
    P.ncomp = sampling == NSR_JPEG_GREY ? 1 : 3;
    P.bpm = P.ncomp == 1 ? 1 : P.hs * P.vs + 2;
    P.mcux = (W + 8 * P.hs - 1) / (8 * P.hs);
    P.mcuy = (H + 8 * P.vs - 1) / (8 * P.vs);
    const long long M = (long long)P.mcux * P.mcuy;
    P.nblk = M * P.bpm;
    if (n * P.nblk > 2147483647ll || (long long)n * H * W > (1ll << 38)) return "too many blocks for one call";
    P.M = (int)M;
    P.pw_y = P.mcux * P.hs * 8;
    P.pw_c = P.mcux * 8;
    P.ph_c = P.mcuy * 8;
    P.cw = (W + P.hs - 1) / P.hs;
    P.ch = (H + P.vs - 1) / P.vs;
    P.poff_c = (long long)P.pw_y * P.mcuy * P.vs * 8;
    P.plane_bytes = P.poff_c + (P.ncomp == 3 ? 2ll * P.pw_c * P.ph_c : 0ll);
    return nullptr;
}

void jpegdec_carve(nsr::JpegDecParams &P, Carve &c) {
    P.coef = c.take<short>(64 * P.n * P.nblk);
    P.planes = c.take<unsigned char>(P.n * P.plane_bytes);
    P.istart = c.take<int>((long long)P.n * (P.M + 1));
    P.nfound = c.take<int>(P.n);
    P.mflags = c.take<int>(P.n);
    P.cstat = c.take<int>((long long)P.n * P.M);
}

}  // namespace

extern "C" {

int nsr_jpegdec_size(int32_t n, int32_t H, int32_t W, int32_t sampling, int64_t max_scan_bytes, int32_t subsequence_bytes,
                     int64_t *workspace_bytes) {
    nsr::JpegDecParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = jpegdec_geometry(n, H, W, sampling, subsequence_bytes, P)) return fail(std::string("nsr_jpegdec_size: ") + e);
    if (max_scan_bytes < 0 || max_scan_bytes > nsr::kJpdMaxScan) return fail("nsr_jpegdec_size: max_scan_bytes must be in [0, 2^28]");
    if (!workspace_bytes) return fail("nsr_jpegdec_size: null pointer");
    *workspace_bytes = carve(jpegdec_carve, P);
    return 0;
}

int nsr_jpegdec_decode(const uint8_t *files, const nsr_jpegdec_frame *descriptors, int32_t n, int32_t H, int32_t W, int32_t sampling,
                       int32_t subsequence_bytes, void *workspace, int64_t workspace_bytes, uint8_t *out, int32_t *status, void *stream) {
    nsr::JpegDecParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = jpegdec_geometry(n, H, W, sampling, subsequence_bytes, P)) return fail(std::string("nsr_jpegdec_decode: ") + e);
    if (n == 0) return 0;
    if (!files || !descriptors || !workspace || !out || !status) return fail("nsr_jpegdec_decode: null pointer");
    if (workspace_bytes < carve(jpegdec_carve, P, workspace)) return fail("nsr_jpegdec_decode: workspace smaller than nsr_jpegdec_size reports");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail("nsr_jpegdec_decode: the workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(descriptors) & 7) return fail("nsr_jpegdec_decode: the descriptors must be 8-byte aligned");
    P.files = files;
    P.desc = descriptors;
    P.out = out;
    P.status = status;
    const int T = nsr::kJpgThreads, scan_lds = nsr::kJpgScanLds + 16;
    const unsigned gx = (unsigned)(P.M < nsr::kJpdMaxGridX ? P.M : nsr::kJpdMaxGridX);
    NSR_LAUNCH(nsr::jpegdec_clear_kernel, dim3(nblk(8ll * n * P.nblk, T)), dim3(T), 0, stream, P);
    NSR_LAUNCH(nsr::jpegdec_markers_kernel, dim3(n), dim3(T), scan_lds, stream, P);
    NSR_LAUNCH(nsr::jpegdec_huffman_kernel, dim3(gx, n), dim3(nsr::kJpdThreads), nsr::kJpdHuffmanLds, stream, P);
    NSR_LAUNCH(nsr::jpegdec_dc_kernel, dim3(gx, n), dim3(T), scan_lds, stream, P);
    NSR_LAUNCH(nsr::jpegdec_idct_kernel, dim3(nblk(n * P.nblk, T)), dim3(T), 0, stream, P);
    NSR_LAUNCH(nsr::jpegdec_color_kernel, dim3(nblk((long long)n * H * W, T)), dim3(T), 0, stream, P);
    return finish("nsr_jpegdec_decode");
}

}  // extern "C"

// ---- PNG decoding (include/nsr.h, "PNG decoding") ----
namespace {

// nullptr: the sizes are valid and P's geometry is filled; else what is wrong with them
const char *png_geometry(int32_t n, int32_t H, int32_t W, int32_t kind, nsr::PngParams &P) {
    if (n < 0 || n > 65535) return "the batch size must be in [0, 65535]";
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return "image sizes must be in [1, 32768]";
    if (kind < NSR_PNG_GREY8 || kind > NSR_PNG_RGBA8) return "kind must be 0 (grey 8), 1 (grey 16), 2 (RGB 8) or 3 (RGBA 8)";
    P.n = n; P.H = H; P.W = W; P.kind = kind;
    P.bpp = kind == NSR_PNG_GREY8 ? 1 : kind == NSR_PNG_GREY16 ? 2 : kind == NSR_PNG_RGB8 ? 3 : 4;
    P.slice = pad16((long long)H * (1 + (long long)W * P.bpp));
    if (n * P.slice > (1ll << 40)) return "too many bytes for one call";
    return nullptr;
}

void png_carve(nsr::PngParams &P, Carve &c) { P.filtered = c.take<unsigned char>(P.n * P.slice); }

}  // namespace

extern "C" {

int nsr_png_size(int32_t n, int32_t H, int32_t W, int32_t kind, int64_t *workspace_bytes) {
    nsr::PngParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = png_geometry(n, H, W, kind, P)) return fail(std::string("nsr_png_size: ") + e);
    if (!workspace_bytes) return fail("nsr_png_size: null pointer");
    *workspace_bytes = carve(png_carve, P);
    return 0;
}

int nsr_png_decode(const uint8_t *streams, const nsr_png_frame *descriptors, int32_t n, int32_t H, int32_t W, int32_t kind,
                   int32_t out_channels, void *workspace, int64_t workspace_bytes, void *out, int32_t *status, void *stream) {
    nsr::PngParams P;
    std::memset(&P, 0, sizeof(P));
    if (const char *e = png_geometry(n, H, W, kind, P)) return fail(std::string("nsr_png_decode: ") + e);
    const bool fits = kind == NSR_PNG_GREY8 ? out_channels == 1 || out_channels == 3 : kind == NSR_PNG_GREY16 ? out_channels == 1
                    : kind == NSR_PNG_RGB8 ? out_channels == 3 : out_channels == 3 || out_channels == 4;
    if (!fits) return fail("nsr_png_decode: out_channels must be 1 or 3 for grey 8, 1 for grey 16, 3 for RGB 8, 3 or 4 for RGBA 8");
    if (n == 0) return 0;
    if (!streams || !descriptors || !workspace || !out || !status) return fail("nsr_png_decode: null pointer");
    if (workspace_bytes < carve(png_carve, P, workspace)) return fail("nsr_png_decode: workspace smaller than nsr_png_size reports");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail("nsr_png_decode: the workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(descriptors) & 7) return fail("nsr_png_decode: the descriptors must be 8-byte aligned");
    if (kind == NSR_PNG_GREY16 && (reinterpret_cast<uintptr_t>(out) & 1)) return fail("nsr_png_decode: a 16-bit out must be 2-byte aligned");
    P.streams = streams;
    P.desc = descriptors;
    P.out = out;
    P.status = status;
    P.out_channels = out_channels;
    const dim3 grid(n), block(nsr::kPngThreads);
    if (int rc = launch_kernel(nsr::png_inflate_kernel, grid, block, nsr::kPngInflateLds, "nsr_png_decode", stream, P)) return rc;
    if (P.bpp == 1) NSR_LAUNCH(nsr::png_unfilter_kernel<1>, grid, block, 0, stream, P);
    else if (P.bpp == 2) NSR_LAUNCH(nsr::png_unfilter_kernel<2>, grid, block, 0, stream, P);
    else if (P.bpp == 3) NSR_LAUNCH(nsr::png_unfilter_kernel<3>, grid, block, 0, stream, P);
    else NSR_LAUNCH(nsr::png_unfilter_kernel<4>, grid, block, 0, stream, P);
    return finish("nsr_png_decode");
}

}  // extern "C"

// ---- frame preparation (include/nsr.h, "Frame preparation") ----
namespace {

constexpr int kFrameMaxSide = 32768;

struct FrameGeometry {
    int Hs, Ws, H, W;
    bool crop, resize;
    float png_depth_scale;
};

// nullptr: the description is valid and G is filled; else what is wrong with it
const char *frame_geometry(const nsr_frame_desc *d, FrameGeometry &G) {
    if (!d) return "null pointer";
    const int32_t sides[4] = {d->color_h, d->color_w, d->depth_h, d->depth_w};
    for (int32_t s : sides)
        if (s < 1 || s > kFrameMaxSide) return "image sizes must be in [1, 32768]";
    if ((d->crop_h == 0) != (d->crop_w == 0) || d->crop_h < 0 || d->crop_w < 0 || d->crop_h > kFrameMaxSide || d->crop_w > kFrameMaxSide)
        return "crop_h and crop_w must both be 0 (no crop_size) or both in [1, 32768]";
    if (d->depth_type != NSR_DEPTH_U16 && d->depth_type != NSR_DEPTH_F32) return "depth_type must be NSR_DEPTH_U16 or NSR_DEPTH_F32";
    G.crop = d->crop_h > 0;
    G.Hs = G.crop ? d->crop_h : d->depth_h;
    G.Ws = G.crop ? d->crop_w : d->depth_w;
    if (d->crop_edge < 0 || 2ll * d->crop_edge >= G.Hs || 2ll * d->crop_edge >= G.Ws) return "crop_edge must be >= 0 and leave at least one pixel";
    G.H = G.Hs - 2 * d->crop_edge;
    G.W = G.Ws - 2 * d->crop_edge;
    G.resize = d->color_h != d->depth_h || d->color_w != d->depth_w;
    G.png_depth_scale = (float)d->png_depth_scale;
    if (!(G.png_depth_scale > 0.f) || !std::isfinite(G.png_depth_scale)) return "png_depth_scale must be positive and finite";
    if (d->has_distortion) {
        if (!(d->fx != 0.0) || !(d->fy != 0.0) || !std::isfinite(d->fx) || !std::isfinite(d->fy))
            return "distortion needs fx and fy that are finite and not 0";
    }
    return nullptr;
}

// the undistorted colour frames (nothing without distortion)
long long frame_ws_bytes(const nsr_frame_desc *d, int32_t B) { return d->has_distortion ? 3ll * B * d->color_h * d->color_w : 0; }

}  // namespace

extern "C" {

int nsr_frame_out_size(const nsr_frame_desc *desc, int32_t *H, int32_t *W) {
    FrameGeometry G;
    if (const char *e = frame_geometry(desc, G)) return fail(std::string("nsr_frame_out_size: ") + e);
    if (!H || !W) return fail("nsr_frame_out_size: null pointer");
    *H = G.H;
    *W = G.W;
    return 0;
}

int64_t nsr_frame_workspace_bytes(const nsr_frame_desc *desc, int32_t B) {
    FrameGeometry G;
    if (B < 0 || frame_geometry(desc, G)) return -1;
    return frame_ws_bytes(desc, B);
}

int nsr_frame_prepare(const void *color_raw, const void *depth_raw, const nsr_frame_desc *desc, int32_t B, float *color, float *depth,
                      void *workspace, int64_t workspace_bytes, void *stream) {
    FrameGeometry G;
    if (const char *e = frame_geometry(desc, G)) return fail(std::string("nsr_frame_prepare: ") + e);
    if (B < 0) return fail("nsr_frame_prepare: negative batch size");
    if (B == 0) return 0;
    if (!color_raw || !depth_raw || !color || !depth) return fail("nsr_frame_prepare: null pointer");
    const long long need = frame_ws_bytes(desc, B);
    if (need > 0 && !workspace) return fail("nsr_frame_prepare: null pointer (workspace, needed with distortion)");
    if (workspace_bytes < need) return fail("nsr_frame_prepare: workspace too small (nsr_frame_workspace_bytes)");
    const int T = nsr::kFrThreads;
    const long long max_items = 2147483647ll * T;

    nsr::FrameParams P;
    std::memset(&P, 0, sizeof(P));
    P.color = static_cast<const unsigned char *>(color_raw);
    if (desc->has_distortion) {
        nsr::UndistortParams U;
        std::memset(&U, 0, sizeof(U));
        U.src = P.color; U.dst = static_cast<unsigned char *>(workspace);
        U.H = desc->color_h; U.W = desc->color_w; U.items = (long long)B * U.H * U.W;
        if (U.items > max_items) return fail("nsr_frame_prepare: too many pixels for one launch");
        U.fx = desc->fx; U.fy = desc->fy; U.cx = desc->cx; U.cy = desc->cy;
        U.k1 = desc->dist[0]; U.k2 = desc->dist[1]; U.p1 = desc->dist[2]; U.p2 = desc->dist[3]; U.k3 = desc->dist[4];
        NSR_LAUNCH(nsr::frame_undistort_kernel, dim3((unsigned)nblk(U.items, T)), dim3(T), 0, stream, U);
        P.color = U.dst;
    }
    P.depth = depth_raw; P.out_color = color; P.out_depth = depth;
    P.Hc = desc->color_h; P.Wc = desc->color_w; P.Hd = desc->depth_h; P.Wd = desc->depth_w;
    P.H = G.H; P.W = G.W; P.edge = desc->crop_edge;
    P.depth_f32 = desc->depth_type == NSR_DEPTH_F32 ? 1 : 0;
    P.bgr = desc->color_bgr ? 1 : 0;
    P.resize = G.resize ? 1 : 0; P.crop = G.crop ? 1 : 0;
    P.stream = (!desc->has_distortion && !G.resize && !G.crop) ? 1 : 0;
    P.png_depth_scale = G.png_depth_scale; P.scale = (float)desc->scale;
    P.nn_h = (float)P.Hd / (float)G.Hs; P.nn_w = (float)P.Wd / (float)G.Ws;
    P.rs_h = (double)P.Hc / (double)P.Hd; P.rs_w = (double)P.Wc / (double)P.Wd;
    P.ac_h = G.Hs > 1 ? (double)(P.Hd - 1) / (double)(G.Hs - 1) : 0.0;
    P.ac_w = G.Ws > 1 ? (double)(P.Wd - 1) / (double)(G.Ws - 1) : 0.0;
    for (int i = 0; i < 256; ++i) P.tab[i] = (float)((double)i / 255.0);
    P.items = (long long)B * P.H * (P.stream ? (P.W + nsr::kFrLane - 1) / nsr::kFrLane : P.W);
    if (P.items > max_items) return fail("nsr_frame_prepare: too many pixels for one launch");
    NSR_LAUNCH(nsr::frame_prepare_kernel, dim3((unsigned)nblk(P.items, T)), dim3(T), 0, stream, P);
    return finish("nsr_frame_prepare");
}

}  // extern "C"

// ---- pose algebra (include/nsr.h, "Pose algebra") ----
extern "C" {

int nsr_tensor_from_camera(const float *rt, int64_t n, int32_t row_floats, float *cam, void *stream) {
    if (n < 0) return fail("nsr_tensor_from_camera: negative count");
    if (row_floats != 12 && row_floats != 16) return fail("nsr_tensor_from_camera: row_floats must be 12 (3x4) or 16 (4x4)");
    if (n == 0) return 0;
    if (!rt || !cam) return fail("nsr_tensor_from_camera: null pointer");
    nsr::PoseFromParams P;
    P.rt = rt; P.n = n; P.row_floats = row_floats; P.cam = cam;
    NSR_LAUNCH(nsr::pose_tensor_from_camera_kernel, dim3(1), dim3(nsr::kPoseThreads), 0, stream, P);
    return finish("nsr_tensor_from_camera");
}

int nsr_pose_predict(float *traj, int64_t n_frames, const int64_t *idx, int32_t const_speed, float *cam, void *stream) {
    if (n_frames < 1) return fail("nsr_pose_predict: the trajectory is empty");
    if (!traj || !idx || !cam) return fail("nsr_pose_predict: null pointer");
    nsr::PosePredictParams P;
    P.traj = traj; P.n_frames = n_frames; P.idx = reinterpret_cast<const long long *>(idx); P.const_speed = const_speed ? 1 : 0; P.cam = cam;
    NSR_LAUNCH(nsr::pose_predict_kernel, dim3(1), dim3(nsr::kPoseThreads), 0, stream, P);
    return finish("nsr_pose_predict");
}

int nsr_pose_commit(const float *hist, int32_t n_iters, float *traj, int64_t n_frames, const int64_t *idx, float *best, void *stream) {
    if (n_iters < 0) return fail("nsr_pose_commit: negative iteration count");
    if (n_frames < 1) return fail("nsr_pose_commit: the trajectory is empty");
    if (n_iters == 0) return 0;
    if (!hist || !traj || !idx) return fail("nsr_pose_commit: null pointer");
    nsr::PoseCommitParams P;
    P.hist = hist; P.n_iters = n_iters; P.traj = traj; P.n_frames = n_frames; P.idx = reinterpret_cast<const long long *>(idx); P.best = best;
    NSR_LAUNCH(nsr::pose_commit_kernel, dim3(1), dim3(nsr::kPoseThreads), 0, stream, P);
    return finish("nsr_pose_commit");
}

int nsr_pose_store(const float *cams, int32_t m, const int64_t *index, float *dst, int64_t n_dst, void *stream) {
    if (m < 0) return fail("nsr_pose_store: negative count");
    if (m == 0) return 0;
    if (n_dst < 1) return fail("nsr_pose_store: the pose table is empty");
    if (!cams || !index || !dst) return fail("nsr_pose_store: null pointer");
    nsr::PoseStoreParams P;
    P.cams = cams; P.m = m; P.index = reinterpret_cast<const long long *>(index); P.dst = dst; P.n_dst = n_dst;
    NSR_LAUNCH(nsr::pose_store_kernel, dim3(1), dim3(nsr::kPoseThreads), 0, stream, P);
    return finish("nsr_pose_store");
}

}  // extern "C"

// ---- trajectory evaluation (include/nsr.h, "Trajectory evaluation") ----
extern "C" {

int nsr_ate_eval(const float *est, const float *gt, int64_t n_frames, const int64_t *last, int32_t B, float scale, double *rec, double *err,
                 void *stream) {
    if (n_frames < 1 || n_frames > (1ll << 24)) return fail("nsr_ate_eval: n_frames must be in [1, 2^24]");
    if (B < 0 || B > (1 << 20)) return fail("nsr_ate_eval: the number of problems must be in [0, 2^20]");
    if (!(scale > 0.f) || scale > 3.0e38f) return fail("nsr_ate_eval: scale must be positive and finite");
    if (B == 0) return 0;
    if (!est || !gt || !last || !rec) return fail("nsr_ate_eval: null pointer");
    nsr::AteParams P;
    P.est = est; P.gt = gt; P.n_frames = n_frames; P.last = reinterpret_cast<const long long *>(last); P.scale = scale; P.rec = rec; P.err = err;
    NSR_LAUNCH(nsr::ate_eval_kernel, dim3((unsigned)B), dim3(nsr::kAteThreads), nsr::kAteLds, stream, P);
    return finish("nsr_ate_eval");
}

int nsr_ate_plot(const float *est, const float *gt, int64_t n_frames, const int64_t *last, float scale, const double *rec, int32_t H, int32_t W,
                 uint8_t *image, void *stream) {
    if (n_frames < 1 || n_frames > (1ll << 24)) return fail("nsr_ate_plot: n_frames must be in [1, 2^24]");
    if (!(scale > 0.f) || scale > 3.0e38f) return fail("nsr_ate_plot: scale must be positive and finite");
    if (H < 1 || W < 1 || H > 32768 || W > 32768 || 3ll * H * W >= (1ll << 31)) return fail("nsr_ate_plot: the image size must be in [1, 32768] with 3 H W below 2^31");
    if (!est || !gt || !last || !rec || !image) return fail("nsr_ate_plot: null pointer");
    nsr::AtePlotParams P;
    P.est = est; P.gt = gt; P.n_frames = n_frames; P.last = reinterpret_cast<const long long *>(last); P.scale = scale; P.rec = rec;
    P.out = image; P.H = H; P.W = W;
    NSR_LAUNCH(nsr::ate_plot_kernel, dim3((unsigned)nblk((long long)H * W, nsr::kPlotThreads)), dim3(nsr::kPlotThreads), nsr::kPlotLds, stream, P);
    return finish("nsr_ate_plot");
}

}  // extern "C"
