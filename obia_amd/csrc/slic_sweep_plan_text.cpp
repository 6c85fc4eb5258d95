// slic_sweep_plan_text.cpp -- obia_test_sweep_plan (include/obia_testing.h): the plan of a batch's sweeps (slic_sweep_plan.hpp) as text,
// one command per line in queue order.  Pure host code: the batch is made up from a table of problem shapes, nothing is launched.
#include <cstdarg>

#include "slic_sweep_plan.hpp"

namespace obia {
namespace {

struct Text {
    std::string s;
    void line(const char *fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        s += buf;
        s += '\n';
    }
};

std::string list(const std::vector<int> &v) {
    std::string s = "{";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? " " : "") + std::to_string(v[i]);
    return s + "}";
}

// the kernel as the source names it
std::string kernel_name(const SlicBatch &b, const SweepStep &s) {
    const std::string cp = std::to_string(b.CP), m = b.masked ? "true" : "false", nch = s.nch == b.CP ? "" : ", " + std::to_string(s.nch);
    switch (s.kernel) {
        case SweepKernel::SpatialRuns: return "slic_spatial_kernel<" + cp + ">";
        case SweepKernel::Lean: return "slic_prepass_kernel<" + cp + ", " + m + ", false>";
        case SweepKernel::LeanFixpt: return "slic_prepass_kernel<" + cp + ", " + m + ", true>";
        case SweepKernel::IgnoreColor: return "slic_assign_kernel<" + cp + ", true, true, false, false>";
        case SweepKernel::FixptSpatial: return "slic_assign_kernel<" + cp + ", true, true, true, false>";
        case SweepKernel::Rawin: return "slic_assign_rawin_kernel<" + cp + ">";
        case SweepKernel::Main: return "slic_assign_kernel<" + cp + ", " + m + ", false, false, false" + nch + ">";
        case SweepKernel::ColLb: return "slic_assign_collb_kernel<" + cp + ", " + m + nch + ">";
        case SweepKernel::SlicZero: return "slic_assign_kernel<" + cp + ", " + m + ", false, false, true>";
        case SweepKernel::Fixpt: return "slic_assign_kernel<" + cp + ", " + m + ", false, true, false>";
    }
    return "?";
}

void write_plan(const SlicBatch &b, const SweepPlan &pl, Text &t) {
    if (pl.no_sweep) { t.line("s0 fill labels"); t.line("no sweep"); return; }
    t.line("batch grp_split %d col_split %d n_shared %d", pl.grp_split, pl.col_split, pl.n_shared);
    if (pl.n_shared > 0)
        t.line("classes %s ap %s at %s mr %s kmax_act %d kmax_mem %d shared_px %.0f", pl.class_span ? "span" : "table", list(pl.ap).c_str(),
               list(pl.at).c_str(), list(pl.mr).c_str(), pl.kmax_act, pl.kmax_mem, pl.shared_px);
    if (pl.fixed_point) t.line("s0 fill bin_stamp tile_lp");
    if (pl.pack_mask) { t.line("s0 upload"); t.line("s0 pack mask grid (%d, %d)", pl.pack_rows, b.nprob); }
    if (pl.fill_first) t.line("s0 fill labels");
    t.line("s0 upload");
    t.line("s0 clear");
    for (const SweepStep &s : pl.steps) {
        const char *pass = s.spatial ? "spatial" : "colour";
        if (s.refill) t.line(pl.fixed_point ? "s0 fill labels tile_lp" : "s0 fill labels");
        if (s.broadcast) t.line("s0 broadcast grid (%d, %d)", cdiv(pl.kmax_mem, 64), pl.n_shared);
        if (s.fork) t.line("fork s0 -> s1");
        for (int i = 0; i < s.nparts; ++i) {
            const SweepPart &q = s.part[i];
            const char *step = s.step_kernel == StepKernel::Lane ? "slic_prep_lane_kernel" : (s.step_kernel == StepKernel::Grouped16 ? "slic_prep_kernel<16>" : "slic_prep_kernel<32>");
            if (s.step_kernel != StepKernel::Lane)
                t.line("s%d step %d %s %s parity %d first %d zmode %d cells [%d, %d)", q.stream, s.sweep_no, pass, step, s.parity, s.first ? 1 : 0, s.zmode, q.cell_base, q.cell_end);
            else if (q.table)
                t.line("s%d step %d %s %s<%d> parity %d first %d zmode %d grid (%d, %d) problems table cells [%d, %d)", q.stream, s.sweep_no, pass, step,
                       b.CP, s.parity, s.first ? 1 : 0, s.zmode, cdiv(q.kmax, 64), q.n_probs, q.cell_base, q.cell_end);
            else
                t.line("s%d step %d %s %s<%d> parity %d first %d zmode %d grid (%d, %d) problems [%d, %d) cells [%d, %d)", q.stream, s.sweep_no, pass, step,
                       b.CP, s.parity, s.first ? 1 : 0, s.zmode, cdiv(q.kmax, 64), q.n_probs, q.p_base, q.p_base + q.n_probs, q.cell_base, q.cell_end);
            if (s.maxdist) t.line("s0 maxdist grid (%d, %d)", pl.maxdist_rows, b.nprob);
            const std::string tiles = q.table ? "tiles table " + std::to_string(q.tile_end) : "tiles [" + std::to_string(q.tile_base) + ", " + std::to_string(q.tile_end) + ")";
            t.line("s%d sweep %d %s %s nch %d %s accumulate %d accum_color %d store %d cache %d slot %d timing %s", q.stream, s.sweep_no, pass,
                   kernel_name(b, s).c_str(), s.nch, tiles.c_str(), s.accumulate, s.accum_color, s.store_labels, s.use_cache, s.counter_slot,
                   s.timing == T_PREPASS ? "prepass" : (s.timing == T_ASSIGN_GRP ? "assign_grp" : "assign"));
        }
        if (s.join) t.line("join s1 -> s0");
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" int obia_test_sweep_plan(const int64_t *problems, int n_problems, const int32_t *settings, int repeat, const int32_t *switches,
                                    const int64_t *residencies, char *text, int64_t text_bytes) {
    if (!settings || !switches || !residencies || !text || text_bytes < 1 || n_problems < 0 || (n_problems > 0 && !problems)) {
        set_error("obia_test_sweep_plan: bad arguments");
        return OBIA_E_INVALID;
    }
    static const unsigned char present[16] = {0};   // stands for device memory that exists: the plan looks at no pointer's target
    SlicBatch b;
    b.C = settings[0]; b.CP = 4 * ((b.C + 3) / 4);
    b.masked = settings[1] != 0;
    b.max_iter = settings[2]; b.prepass_iter = settings[3]; b.prepass_only = settings[4] != 0;
    b.exit_on_fixed_point = settings[5] != 0; b.slic_zero = settings[6] != 0; b.direct = settings[7] != 0;
    b.col_lb = settings[8] != 0;
    if (b.col_lb) b.d_fbox = reinterpret_cast<float *>(const_cast<unsigned char *>(present));
    b.fuse_features = settings[9] != 0;
    if (b.fuse_features) { b.raw_src = reinterpret_cast<const float *>(present); b.d_keys = reinterpret_cast<const unsigned *>(present); }
    if (b.masked) b.d_mask = const_cast<unsigned char *>(present);
    if (b.masked && settings[10]) b.d_mask4 = reinterpret_cast<unsigned *>(const_cast<unsigned char *>(present));
    b.nprob = n_problems;
    long long tiles_all = 0;
    for (int p = 0; p < n_problems; ++p) {   // the layout as slic_plan_layout and slic_plan_and_seed leave it
        const int64_t *r = problems + 7 * (size_t)p;
        SlicProblem P = SlicProblem();
        P.H = (int)r[0]; P.W = (int)r[1]; P.K = (int)r[2]; P.sy = (int)r[3]; P.sx = (int)r[4]; P.n_valid = (int)r[5];
        if (P.H < 1 || P.W < 1 || P.K < 0 || P.sy < 1 || P.sx < 1) { set_error("obia_test_sweep_plan: bad problem %d", p); return OBIA_E_INVALID; }
        P.ncy = cdiv(P.H, P.sy); P.ncx = cdiv(P.W, P.sx);
        P.tiles_x = cdiv(P.W, SWEEP_TW); P.tiles_y = cdiv(P.H, SWEEP_TH);
        P.spatial_w = 1.0f; P.sp_y = P.sp_x = 1.0f; P.direct = b.direct ? 1 : 0;
        P.cent_off = b.total_cent; P.cell_off = b.total_cells; P.tile_off = (int)tiles_all; P.pix_off = b.total_pix;
        b.total_cent += P.K; b.total_cells += P.ncy * P.ncx; tiles_all += P.tiles_x * P.tiles_y; b.total_pix += (long long)P.H * P.W;
        b.total_tiles = std::max(b.total_tiles, P.tiles_x * P.tiles_y);
        b.probs.push_back(P);
        b.grid_n.push_back(r[6]);
    }
    b.total_tiles_all = tiles_all > 0 ? tiles_all : 1;
    if (b.total_cells < 1) b.total_cells = 1;
    SweepSwitches sw;
    sw.debug_sync = switches[0] != 0; sw.prep_grouped = switches[1] != 0; sw.prepass_visits = switches[2] != 0;
    sw.prepass_share = switches[3] != 0; sw.prepass_groups = switches[4]; sw.sweep_groups = switches[5];
    SweepResidencies res;
    res.spatial = residencies[0]; res.colour = residencies[1];
    SweepPlan pl;
    OBIA_TRY(plan_sweeps(b, repeat != 0, sw, sweep_grouping(b, repeat != 0, sw), res, pl));
    Text t;
    write_plan(b, pl, t);
    if ((int64_t)t.s.size() + 1 > text_bytes) { set_error("obia_test_sweep_plan: the text needs %zu bytes", t.s.size() + 1); return OBIA_E_INVALID; }
    memcpy(text, t.s.c_str(), t.s.size() + 1);
    return OBIA_OK;
}
