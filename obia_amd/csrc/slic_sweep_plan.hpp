// slic_sweep_plan.hpp -- what a batch's sweeps launch, decided as data (host code only: no HIP call, no arena, no context).
// plan_sweeps() computes a SweepPlan from the batch; slic_sweep.hip issues it in one loop over its steps and their parts;
// obia_test_sweep_plan (include/obia_testing.h) writes it out as text, which tests/test_sweep_plan_cpu.py pins without a GPU.
#pragma once
#include <cstdlib>

#include "slic.hpp"

namespace obia {

// The developer switches of the sweep driver, read once per batch (read_sweep_switches).
//   debug_sync      OBIA_DEBUG_SYNC: stage-by-stage synchronisation (context.cpp: debug_sync) and the problem table on stderr
//   prep_grouped    OBIA_PREP_GROUPED (A/B timing, tests/test_gpu_prep_kernels.py): the 16-lanes-per-centroid step kernel
//   prepass_visits  OBIA_PREPASS_VISITS (A/B timing, tests/test_gpu_prepass_runs.py): the spatial pre-pass by pixel visits, not runs
//   prepass_share   OBIA_PREPASS_SHARE=0 (A/B timing, tests/test_gpu_prepass_share.py): no shared pre-pass
//   prepass_groups  OBIA_PREPASS_GROUPS (tests/test_gpu_prepass_groups.py): 0 never, 2 at any size, else 1 (the size threshold decides)
//   sweep_groups    OBIA_SWEEP_GROUPS (tests/test_gpu_sweep_groups.py): the same for the colour pass, independent of the other
struct SweepSwitches {
    bool debug_sync = false, prep_grouped = false, prepass_visits = false, prepass_share = true;
    int prepass_groups = 1, sweep_groups = 1;
};
inline SweepSwitches read_sweep_switches() {
    const auto set = [](const char *name) { return std::getenv(name) != nullptr; };
    const auto mode = [](const char *name) { const char *e = std::getenv(name); return !e ? 1 : (e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1)); };
    const char *share = std::getenv("OBIA_PREPASS_SHARE");
    return SweepSwitches{set("OBIA_DEBUG_SYNC"), set("OBIA_PREP_GROUPED"), set("OBIA_PREPASS_VISITS"), !(share && share[0] == '0'),
                         mode("OBIA_PREPASS_GROUPS"), mode("OBIA_SWEEP_GROUPS")};
}

// Workgroups the device holds at once of slic_spatial_kernel and of the batch's colour kernel; asked for by the caller only when
// SweepGrouping says so, 0 otherwise (not looked at)
struct SweepResidencies { long long spatial = 0, colour = 0; };

// The kernel of a sweep:
//   SpatialRuns    slic_spatial_kernel<CP>: a spatial-only sweep that stores no labels and keeps no fixed-point cache, decided by runs
//   Lean           slic_prepass_kernel<CP, M, false>: the same sweep pixel by pixel (it stores labels, or OBIA_PREPASS_VISITS)
//   LeanFixpt      slic_prepass_kernel<CP, M, true>
//   IgnoreColor    slic_assign_kernel<CP, true, true, false, false>: the last pre-pass sweep, which folds colours
//   FixptSpatial   slic_assign_kernel<CP, true, true, true, false>: the same under exit_on_fixed_point
//   Rawin          slic_assign_rawin_kernel<CP>: the same with the fused feature pass
//   Main           slic_assign_kernel<CP, M, false, false, false, NCH>
//   ColLb          slic_assign_collb_kernel<CP, M, NCH>: low compactness, with the colour-box bound
//   SlicZero       slic_assign_kernel<CP, M, false, false, true>
//   Fixpt          slic_assign_kernel<CP, M, false, true, false>
enum class SweepKernel { SpatialRuns, Lean, LeanFixpt, IgnoreColor, FixptSpatial, Rawin, Main, ColLb, SlicZero, Fixpt };
enum class StepKernel { Lane, Grouped16, Grouped32 };   // slic_prep_lane_kernel<CP>, or slic_prep_kernel<16 / 32> (OBIA_PREP_GROUPED)

// What one launch pair (centroid step, sweep) covers.  The step's launch steps the problems [p_base, p_base + n_probs), or the
// n_probs the class table names (table: through SweepPlan::ap and at), in a grid of cdiv(kmax, 64) x n_probs -- kmax: most centroids
// of one of its problems -- and resets the bins [cell_base, cell_end) of the next sweep's buffer; the sweep covers the tiles
// [tile_base, tile_end), or the tile_end tiles the class table names.  stream 0: the context's, 1: the side stream.
struct SweepPart {
    int p_base = 0, n_probs = 0, kmax = 1, tile_base = 0, tile_end = 0, cell_base = 0, cell_end = 0, stream = 0;
    bool table = false;
};

// One sweep with the centroid step in front of it.
//   sweep_no, parity   sweep ids start at 1; the bin buffer the sweep reads (the step resets the other)
//   spatial            a sweep of the spatial-only pre-pass of a masked batch (else: of the colour pass)
//   zmode              SLIC-zero: 2 the per-cluster colour scale restarts at 1, 1 it is carried, 0 off
//   refill             in front: labels back to the fill value (and tile_lp cleared under exit_on_fixed_point)
//   broadcast          in front: slic_prepass_broadcast_kernel (shared pre-pass)
//   maxdist            behind the centroid step: slic_maxdist_kernel
//   counter_slot       of the pixel counters: 0 colour sweeps, 256 pre-pass sweeps
//   timing             T_ASSIGN, T_PREPASS, or T_ASSIGN_GRP (a colour sweep of one window group)
//   fork, join         in front of the step the side stream waits for the context's; behind the sweep the reverse
//   nparts, part       one part, or the two window groups
struct SweepStep {
    int sweep_no = 0, parity = 0, zmode = 0;
    bool spatial = false, first = false, refill = false, broadcast = false, maxdist = false, fork = false, join = false;
    StepKernel step_kernel = StepKernel::Lane;
    SweepKernel kernel = SweepKernel::Main;
    int nch = 0, accumulate = 0, accum_color = 0, store_labels = 0, use_cache = 0, counter_slot = 0, timing = T_ASSIGN, nparts = 1;
    SweepPart part[2];
};

// A batch's sweeps.
//   no_sweep               fill only: every pixel keeps the fill value
//   fill_first             labels filled up front
//   pack_mask, pack_rows   d_mask -> d_mask4 (mask_pack4_kernel) and its grid.x;  maxdist_rows: grid.x of slic_maxdist_kernel
//   fixed_point            the fixed-point state exists and bin_stamp / tile_lp are cleared up front
//   n_shared ... mr        shared pre-pass: the problems that run the shared sweeps (ap) and their tiles (at) -- a span when they are
//                          consecutive (class_span), else tables --, {member, representative} of every problem that does not (mr), the
//                          most centroids among either, the pixel-sweeps covered by a representative's sweeps and not evaluated
//   grp_split, col_split   > 0: the groups of the pre-pass / the colour pass are the problems [0, split) and [split, nprob)
struct SweepPlan {
    bool no_sweep = false, fill_first = false, pack_mask = false, fixed_point = false, class_span = false;
    int pack_rows = 1, maxdist_rows = 1, n_shared = 0, kmax_act = 1, kmax_mem = 1, grp_split = 0, col_split = 0;
    std::vector<int> ap, at, mr;
    double shared_px = 0.0;
    std::vector<SweepStep> steps;
};

// Two window groups: the problems [0, split) and [split, nprob), consecutive and balanced by sweep tiles, a tie going
// to the later split; 0 when the batch cannot be split.  One choice for the grouped pre-pass and the grouped colour pass.
inline int group_split(const SlicBatch &b) {
    int split = 0;
    long long best = -1;
    for (int p = 1; p < b.nprob; ++p) {
        const long long t0 = b.probs[p].tile_off, t1 = b.total_tiles_all - t0, d = t0 > t1 ? t0 - t1 : t1 - t0;
        if (t0 > 0 && t1 > 0 && (best < 0 || d <= best)) { best = d; split = p; }
    }
    return split;
}
// sweep tiles of the smaller group
inline long long group_min_tiles(const SlicBatch &b, int split) {
    const long long t0 = b.probs[split].tile_off, t1 = b.total_tiles_all - t0;
    return t0 < t1 ? t0 : t1;
}

// The colour kernel of the batch's colour sweeps (SLIC-zero only changes the colour sweeps -- the spatial pre-pass computes no colour
// term -- and is not combined with the fixed-point cache: the per-cluster scale changes after the records were compared)
inline SweepKernel colour_sweep_kernel(const SlicBatch &b) {
    if (b.slic_zero) return SweepKernel::SlicZero;
    if (b.exit_on_fixed_point) return SweepKernel::Fixpt;
    return (b.col_lb && b.d_fbox) ? SweepKernel::ColLb : SweepKernel::Main;
}

// Sweep counts, sharing and grouping: what every other decision starts from.
//   none          no sweep at all
//   passes        maskSLIC: spatial-only pre-pass first (slic_superpixels.py:310-314)
//   pre_iter      sweeps of the pre-pass: max_iter like every pass, unless the stage entry asks for another count (obia_slic_stages::prepass_iters)
//   store_all     false: only the very last sweep stores its labels (the others' labels are dead stores unless a valid pixel is reached by
//                 no window -- see the label stage of the sweep); true: every sweep stores, the reference's literal behaviour, needed by
//                 the fixed-point replay (labels "already in place"), by SLIC-zero (its max-colour-distance pass reads the last assignment)
//                 and by the repeat
//   n_shared, share_rep   slic_prepass_classes, when the pre-pass is shared
//   split         group_split, when a grouping is eligible
//   pre_ok, col_ok        every condition of the grouping holds but the size threshold
//   pre_asks, col_asks    ... and the switch leaves the decision to the threshold: the caller asks for the residency
//
// Shared pre-pass (slic_prepass_broadcast_kernel): the sweeps of the pre-pass but the last, and the centroid steps between them,
// run for the first problem of every class only (slic_prepass_classes).  Not when every sweep stores its labels (the repeat,
// exit_on_fixed_point, SLIC-zero), with a `spacing`, for the stage entry's pre-pass variants, or when no class has a second member:
// the path without sharing, unchanged.  External seeds (seeding="skimage" among them) form no class.
//
// Two window groups in flight: the spatial-only sweeps of the pre-pass (slic_spatial_kernel) and the centroid steps
// in front of them read and write nothing of another problem of the batch -- centroid and accumulator records, bins, candidate
// lists, reference positions, rebuild requests and the packed mask are all indexed through the problem; the two batch-wide words
// are the pixel counters (integer atomics) and the orphan flag (every writer stores 1).  So the batch's problems are split into
// two groups of consecutive problems, balanced by sweep tiles, and each runs its own chain step -> sweep -> step -> ...: group 0
// on the context's stream, group 1 on the side stream, forked behind the fills and joined in front of the step of the last
// pre-pass sweep, which runs on the whole batch as always.  A group's centroid step (a launch bound by wave dispatch that leaves
// the GPU all but empty) and its launch boundaries then hide behind the other group's sweep.  A step resets the next sweep's bins
// of ITS group only: the other group may be one sweep behind and still reading that buffer.  Sweep numbers (list stamps, the
// parity of the bin buffers) advance alike in both groups.  Not for a batch that shares its pre-pass (n_shared > 0), not when
// every sweep stores its labels (the repeat among them), not under the pre-pass developer switches, not under OBIA_DEBUG_SYNC (the
// stage-by-stage synchronisation watches one stream).  By default only when each group fills the device at least once (the
// residency of slic_spatial_kernel): below that a launch does not fill it and the split buys nothing.
//
// The colour pass runs the same way (col_split): each group its chain step -> colour sweep for all max_iter sweeps, forked behind
// the last whole-batch launch in front of the first colour-pass step -- the last pre-pass sweep of a masked batch (the pre-pass
// broadcast and that sweep stay whole-batch), the clears of an unmasked one -- and joined behind each group's last sweep, the one
// that stores its labels, in front of the counters' read-back.  The colour kernels (the main one in every padding variant and the
// low-compactness one) share nothing more than the spatial ones: the colour boxes are read-only and indexed through P.fb_off, the
// planes and labels through P.pix_off.  A batch that shares its PRE-PASS is eligible: its colour pass shares nothing.  Needs two
// sweeps at least; by default each group must hold one residency of the colour kernel it launches.
struct SweepGrouping {
    bool none = true, store_all = false, pre_ok = false, col_ok = false, pre_asks = false, col_asks = false;
    int passes = 1, pre_iter = 0, total_sweeps = 0, n_shared = 0, split = 0;
    std::vector<int> share_rep;
};
inline SweepGrouping sweep_grouping(const SlicBatch &b, bool repeat, const SweepSwitches &sw) {
    SweepGrouping g;
    g.none = b.total_tiles <= 0 || b.max_iter <= 0;
    g.passes = (b.masked && !b.prepass_only) ? 2 : 1;
    g.pre_iter = (b.masked && b.prepass_iter > 0) ? b.prepass_iter : b.max_iter;
    g.total_sweeps = b.masked ? g.pre_iter + (g.passes - 1) * b.max_iter : b.max_iter;
    g.store_all = repeat || b.exit_on_fixed_point || b.slic_zero;
    if (g.none) return g;
    if (sw.prepass_share && b.masked && g.passes == 2 && g.pre_iter >= 2 && b.prepass_iter <= 0 && !g.store_all && !b.direct && !sw.prep_grouped)
        g.n_shared = slic_prepass_classes(b.probs, b.grid_n, g.share_rep);
    if (!g.store_all && !sw.prepass_visits && !sw.prep_grouped && !b.direct && b.nprob >= 2 && !sw.debug_sync) {
        g.split = group_split(b);
        g.pre_ok = g.split > 0 && sw.prepass_groups != 0 && g.n_shared == 0 && b.masked && g.pre_iter >= 2;
        g.col_ok = g.split > 0 && sw.sweep_groups != 0 && !(b.masked && b.prepass_only) && b.max_iter >= 2;
        g.pre_asks = g.pre_ok && sw.prepass_groups != 2;
        g.col_asks = g.col_ok && sw.sweep_groups != 2;
    }
    return g;
}

// The plan of a batch's sweeps.  repeat: the batch runs again from the seeds with every sweep storing its labels.  g: sweep_grouping
// of the same arguments (the caller has it: it says which residencies to ask for).  Refuses (error text set, plan unusable) a window
// of 2^22 pixels or wider and fuse_features on a batch that cannot take it.
inline int plan_sweeps(const SlicBatch &b, bool repeat, const SweepSwitches &sw, const SweepGrouping &g, const SweepResidencies &res, SweepPlan &pl) {
    pl = SweepPlan();
    pl.no_sweep = g.none;
    if (g.none) return OBIA_OK;
    // the sweep addresses a footprint's pixels as a 64-bit wave-uniform base plus a 32-bit lane offset (16 rows x W x 64 B)
    for (auto &P : b.probs)
        if (P.W >= (1 << 22)) { set_error("rasters / tile windows wider than 4194303 pixels are not supported (got %d)", P.W); return OBIA_E_UNSUPPORTED; }
    if (b.fuse_features && (!b.masked || b.exit_on_fixed_point || b.slic_zero || b.direct || b.col_lb || b.C != b.CP || b.CP > 12 || !b.raw_src || !b.d_keys)) {
        set_error("fused feature pass on a batch that cannot take it");   // (slic_fuse_features decides; nothing else may set the flag)
        return OBIA_E_INVALID;
    }
    int maxh = 1;
    for (auto &P : b.probs) maxh = std::max(maxh, P.H);
    // the packed mask of the sweeps (problems whose mask hides nothing never read it); the tiler's mask kernel writes it on the way
    // (tiling.hip: tile_mask_kernel<true>)
    pl.pack_mask = b.masked && b.d_mask && !b.d_mask4;
    pl.pack_rows = (int)grids::slic_mask_pack(maxh, b.nprob).x.n;
    pl.maxdist_rows = (int)grids::slic_maxdist(maxh, b.nprob).x.n;
    pl.fixed_point = b.exit_on_fixed_point;
    // The fill value survives in exactly one kind of pixel: a valid one that no window reached ("orphan").  When only the last sweep
    // stores, such a pixel raises the flag and the caller repeats the batch (slic_sweeps_settle) -- unless the batch has ONE sweep in
    // all, where the fill value is what the reference keeps.  Every other pixel is written by the last sweep (masked ones included):
    // the 1.2 GB fill of a bench batch is skipped on the common path.
    pl.fill_first = g.store_all || g.total_sweeps <= 1;
    if (g.pre_ok && (sw.prepass_groups == 2 || group_min_tiles(b, g.split) >= res.spatial)) pl.grp_split = g.split;
    if (g.col_ok && (sw.sweep_groups == 2 || group_min_tiles(b, g.split) >= res.colour)) pl.col_split = g.split;

    // the part that covers the problems [p0, p1)
    const auto span = [&b](int p0, int p1, int stream) {
        SweepPart q;
        q.p_base = p0; q.n_probs = p1 - p0; q.stream = stream;
        for (int p = p0; p < p1; ++p) q.kmax = std::max(q.kmax, b.probs[p].K);
        q.tile_base = b.probs[p0].tile_off; q.tile_end = p1 < b.nprob ? b.probs[p1].tile_off : (int)b.total_tiles_all;
        q.cell_base = b.probs[p0].cell_off; q.cell_end = p1 < b.nprob ? b.probs[p1].cell_off : b.total_cells;
        return q;
    };
    const SweepPart whole = span(0, b.nprob, 0);
    SweepPart shared = whole;   // the representatives of a shared pre-pass: their steps still reset the bins of the whole batch
    pl.n_shared = g.n_shared;
    pl.kmax_act = g.n_shared > 0 ? 1 : whole.kmax;
    if (g.n_shared > 0) {
        for (int p = 0; p < b.nprob; ++p) {
            const SlicProblem &P = b.probs[p];
            if (g.share_rep[p] == p) {
                pl.ap.push_back(p);
                for (int t = 0; t < P.tiles_x * P.tiles_y; ++t) pl.at.push_back(P.tile_off + t);
                pl.kmax_act = std::max(pl.kmax_act, P.K);
            } else {
                pl.mr.push_back(p); pl.mr.push_back(g.share_rep[p]);
                pl.kmax_mem = std::max(pl.kmax_mem, P.K);
                pl.shared_px += (double)P.H * (double)P.W * (double)(g.pre_iter - 1);
            }
        }
        // consecutive problems: consecutive tiles, no table in front of a tile
        pl.class_span = pl.ap.back() - pl.ap.front() + 1 == (int)pl.ap.size();
        shared = span(pl.ap.front(), pl.ap.back() + 1, 0);
        shared.cell_base = 0; shared.cell_end = b.total_cells;
        if (!pl.class_span) { shared.table = true; shared.n_probs = (int)pl.ap.size(); shared.kmax = pl.kmax_act; shared.tile_base = 0; shared.tile_end = (int)pl.at.size(); }
    }
    const bool fixpt = b.exit_on_fixed_point;
    pl.steps.reserve((size_t)g.total_sweeps);
    int sweep_no = 0;
    for (int pass = 0; pass < g.passes; ++pass) {
        const bool spatial = b.masked && pass == 0, last_pass = pass == g.passes - 1;
        const int iters = spatial ? g.pre_iter : b.max_iter;
        for (int it = 0; it < iters; ++it) {
            const bool last_it = it == iters - 1, very_last = last_pass && last_it;
            SweepStep s;
            s.parity = sweep_no & 1;
            s.sweep_no = ++sweep_no;
            s.spatial = spatial;
            s.first = sweep_no == 1;
            // SLIC-zero: the per-cluster colour scale restarts at 1 with the colour pass and is carried afterwards
            s.zmode = (b.slic_zero && !spatial) ? (it == 0 ? 2 : 1) : 0;
            // the main pass is a second call of _slic_cython (slic_superpixels.py:310-318): `nearest` starts from the fill value again,
            // a pixel no window reaches in its first sweep does not inherit a pre-pass label.  (Only when the pre-pass stored labels at
            // all: otherwise the fill of the batch's start is still in place.)  exit_on_fixed_point: no tile may replay "labels already
            // in place" across the refill -- every tile is evaluated by the first sweep of the main pass
            s.refill = pass > 0 && it == 0 && g.store_all;
            // shared pre-pass: this sweep and the step in front of it run for the representatives only; in front of the step of the
            // last pre-pass sweep the other members receive what they skipped
            const bool shared_sweep = g.n_shared > 0 && spatial && !last_it;
            s.broadcast = g.n_shared > 0 && spatial && last_it;
            s.maxdist = s.zmode == 1;   // the centroids just moved: raise max_dist_color from the assignment of the last sweep
            s.step_kernel = !sw.prep_grouped ? StepKernel::Lane : (acc_record_qwords(b.CP) == 16 ? StepKernel::Grouped16 : StepKernel::Grouped32);
            s.accumulate = very_last ? 0 : 1;   // the update after the very last sweep is never read: skip its accumulation
            s.accum_color = (!spatial || last_it) ? 1 : 0;
            s.store_labels = g.store_all ? 2 : (very_last ? 1 : 0);   // (see slic_sweeps_settle: the orphan flag)
            // the last pre-pass sweep is the only one of its pass that folds colours (they seed the main pass): the caches written by
            // the earlier pre-pass sweeps hold no colour sums, so it evaluates every tile
            s.use_cache = (spatial && last_it) ? 0 : 1;
            // fused feature pass: the last pre-pass sweep -- the first reader of the planes -- writes them from the raster (RAWIN).  Not
            // in the repeat: the first run has written them
            if (b.fuse_features && !repeat && spatial && last_it) s.kernel = SweepKernel::Rawin;
            else if (spatial && !s.accum_color) s.kernel = fixpt ? SweepKernel::LeanFixpt : ((s.store_labels || sw.prepass_visits) ? SweepKernel::Lean : SweepKernel::SpatialRuns);
            else if (spatial) s.kernel = fixpt ? SweepKernel::FixptSpatial : SweepKernel::IgnoreColor;
            else s.kernel = colour_sweep_kernel(b);
            // channels that exist: C of the CP = 4 * ceil(C / 4) the planes and records hold.  The two kernels that run 9 of every 10
            // sweeps come in a variant per padding (slic_assign_body: NCH); the others treat the padded channels like real ones.
            s.nch = (s.kernel == SweepKernel::Main || s.kernel == SweepKernel::ColLb) ? b.C : b.CP;
            s.counter_slot = spatial ? 256 : 0;
            // a sweep as two window groups: a pre-pass sweep but the last, or any sweep of a grouped colour pass
            const bool pre_groups = pl.grp_split > 0 && spatial && !last_it, col_groups = pl.col_split > 0 && !spatial;
            s.timing = spatial ? T_PREPASS : (col_groups ? T_ASSIGN_GRP : T_ASSIGN);
            s.part[0] = shared_sweep ? shared : whole;
            if (pre_groups || col_groups) {
                const int split = col_groups ? pl.col_split : pl.grp_split;
                s.fork = it == 0;
                s.join = it == (col_groups ? iters - 1 : iters - 2);
                s.nparts = 2;
                s.part[0] = span(0, split, 0);
                s.part[1] = span(split, b.nprob, 1);
            }
            pl.steps.push_back(s);
        }
    }
    return OBIA_OK;
}

}  // namespace obia
