// slic_spatial.hip -- the spatial-only pre-pass sweeps of maskSLIC (nine of the ten pre-pass sweeps) decided by RUNS on pixel
// rows instead of by pixels.  Part of the translation unit of slic_sweep.hip (included there: it shares the tile machinery --
// candidate lists, XCD grouping, the packed LDS accumulators -- and falls back to slic_assign_body for the tiles named below).
//
// What such a sweep has to produce is n, sum(y), sum(x) per centroid and nothing else (no labels, no colours; the distance of
// a pixel does not outlive the sweep).  The winner of a pixel is the lexicographic minimum of (d, k) over the centroids whose
// window holds it, d = fl(fl(fl(ty^2) + fl(tx^2)) * w), ty = fl(cy - y), tx = fl(cx - x).  Along a pixel row the winners come
// in a handful of runs, so a lane owns a 16-pixel ROW SEGMENT (a wave: the 16 rows x 4 segments of its band) and evaluates the
// reference's float expression only at the two ends of the segment and at four pixels around the one crossing it predicts;
// everything between two evaluated pixels is handed to the common winner of both -- but only under the margin proven below.
// Whatever is not proven (ties, a third run, a near-horizontal bisector, an end no window reaches) goes to a per-wave queue and
// is decided pixel by pixel, sixteen lanes per queued range, with the reference's expression and tie rule.
//
// ---- the margin (every pixel that is NOT evaluated with the reference's expression is decided under it) ----------------------
// Row y, segment ends a < b (both evaluated), candidates C = the survivors of the footprint's pruning (below).  For c in C whose
// window holds the row, dt_c(x) is the float distance and D_c(x) = (cy_c - y)^2 + (cx_c - x)^2 the exact one, centroid coordinates
// taken as the real numbers their floats are.  With u = 2^-24 and 2^-30 <= w <= 2^90 (checked: other weights take the pixel path;
// w is 1 / step^2 times the squared power-of-two prescale of the features, slic_prescale):
//   (E)  dt_c(x) = D_c(x) w (1 + e) + h,  |e| <= 6u,  |h| <= 2^-94 w.
//        y and x are integers below 2^24: exact as floats.  ty carries one rounding (a subnormal difference is exact), ty^2 two more
//        of ty's and one of its own, the sum one, the product one: (1 + u)^5 - 1 < 6u.  An underflowing square or product adds at
//        most 2^-126 each (flushed or not): two squares times w(1 + u), and the product's own 2^-126 <= 2^-96 w.
//   Let A win both ends (so its window, an interval in x, holds the whole segment) with d1_e = dt_A(e), and let
//   d2_e = min over c != A of dt_c(e), c evaluated at e whether or not its x-window holds e (a candidate that is absent from a
//   pixel can only lose it: extending it is conservative).  The test is
//   (T)  min(d2_a - d1_a, d2_b - d1_b) > 2^-19 max(d1_a, d1_b) + 2^-60 w   (float arithmetic, max(d1) finite).
//   For B != A put g(x) = (D_B(x) - D_A(x)) w: AFFINE in x on the row (the x^2 terms cancel), so g(x) >= min(g(a), g(b)) inside the
//   segment; D_A is convex in x, so D_A(x) w <= max(D_A(a), D_A(b)) w =: M <= max(d1)(1 + 7u) + 2^-93 w.
//   From (E) at an end: g(e) >= dt_B(e)(1 - 6u) - dt_A(e)(1 + 7u) - 2^-92 >= (d2_e - d1_e)(1 - 6u) - 13u d1_e - 2^-92 w.
//   (T) gives d2_e - d1_e > 32u max(d1) + 2^-60 w up to one rounding of the subtraction and two of the right side (factor
//   1 - 4u), hence g(x) > 18u max(d1) + 2^-61 w > 12.1u M + 2^-92 w for every x of the segment.  And g(x) > 12.1u D_A(x) w + 2^-92 w
//   implies D_B w (1 - 6u) - h > D_A w (1 + 6u) + h, i.e. dt_B(x) > dt_A(x) STRICTLY by (E): A wins x whatever the indices.
//   A tie (d2 = d1), a candidate that beats A where its window does not reach (d2 < d1) or an unassigned end (d1 = inf) fails (T).
//
// ---- pruning ------------------------------------------------------------------------------------------------------------------
// Per 16 x 16 footprint, one candidate per lane (the footprint lists of the tile's candidate list): lb = the reference expression
// at the footprint point nearest to the centroid, ub = the same expression with the largest |ty| and |tx| of the footprint, for
// a candidate whose window covers the whole footprint (+inf otherwise).  Every operation is monotone, so lb <= dt_c(p) <= ub
// for every pixel p of the footprint.  A candidate with lb > min(ub) loses every pixel strictly to the covering candidate that
// attains the minimum: dropped; lb == min(ub) stays (it could tie on k).  A second test drops what that candidate beats at the
// four corners of the footprint under the margin (next to the code).  The survivors are written in slot order = ascending k, so
// walking them with a strict `<` IS the reference's tie rule (lowest k wins).
//
// Tiles that keep the pixel-by-pixel kernel body (workgroup-uniform): no candidate list (the first sweep builds them; a tile
// with more than SWEEP_MAXC candidates never has one and ends in slow_tile()), a list whose rebuild was requested, `spacing` != 1
// (the direct path), a weight outside [2^-30, 2^90].  A valid pixel that no window reaches raises the orphan flag exactly as
// before (this kernel only runs sweeps that store no labels: the host then repeats the batch with every sweep storing).

#ifdef OBIA_RUN_STATS
// Diagnostic build only (tools/build_variant.sh rs -DOBIA_RUN_STATS, tools/prepass_run_stats.py): totals over every wave of the run
// kernel -- [0] waves, [1] row segments with a valid pixel, [2] candidates they walked, [3] segments proven from their two ends,
// [4] segments that looked for one crossing, [5] queued ranges, [6] queued pixels, [7] runs added, [8..12] ticks (s_memtime):
// staging, pruning, walk, queue, barrier + flush.
__device__ unsigned long long g_run_stats[16];
#define RS_DECL unsigned long long rs_t = clock64(); unsigned rs_c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define RS_COUNT(i, v) rs_c[i] += (unsigned)(v);
#define RS_TICK(i) { const unsigned long long rs_n = clock64(); if ((threadIdx.x & 63) == 0) atomicAdd(&g_run_stats[i], rs_n - rs_t); rs_t = rs_n; }
#define RS_FLUSH { for (int rs_i = 1; rs_i < 8; ++rs_i) { unsigned rs_v = rs_c[rs_i]; for (int rs_o = 32; rs_o; rs_o >>= 1) rs_v += __shfl_xor(rs_v, rs_o); \
                   if ((threadIdx.x & 63) == 0) atomicAdd(&g_run_stats[rs_i], (unsigned long long)rs_v); } if ((threadIdx.x & 63) == 0) atomicAdd(&g_run_stats[0], 1ull); }
extern "C" void obia_debug_run_stats(unsigned long long *out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_run_stats), sizeof(unsigned long long) * 16);
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_run_stats), z, sizeof(z)); }
}
#else
#define RS_DECL
#define RS_COUNT(i, v)
#define RS_TICK(i)
#define RS_FLUSH
#endif

constexpr float RUN_REL = 0x1p-19f, RUN_ABS = 0x1p-60f, RUN_W_LO = 0x1p-30f, RUN_W_HI = 0x1p90f;

template <int CP>
__device__ __forceinline__ void slic_spatial_tile(const SlicProblem &P, int gtile, int tile, int l_n, const unsigned *__restrict__ mask4,
                                                  const float *__restrict__ cent, unsigned long long *__restrict__ acc, int RQ,
                                                  unsigned long long *__restrict__ px_counter, int *__restrict__ orphan_flag,
                                                  const int *__restrict__ tl_k, const unsigned *__restrict__ tl_fp) {
    constexpr int RS = CENT_REC + CP;
    constexpr int NW = NT / 64;
    constexpr unsigned INF_BITS = 0x7f800000u;
    __shared__ __attribute__((aligned(16))) float r_hdr[MAXC][CENT_REC];   // staged headers, slot = rank (ascending k)
    __shared__ int r_k[MAXC];
    __shared__ unsigned long long r_acc[MAXC];             // n | sum(y - ty0) << 16 | sum(x - tx0) << 40 (see slic_assign_body)
    __shared__ unsigned char r_surv[NW][SWEEP_TW / FB][64];   // survivors of the pruning, per wave and footprint, ascending slot
    __shared__ unsigned r_q[NW][128];                      // ranges left to the pixel-by-pixel pass (two per lane at most)

    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ty0 = (tile / P.tiles_x) * SWEEP_TH, tx0 = (tile % P.tiles_x) * SWEEP_TW;
    const float w = P.spatial_w;
    RS_DECL
    if (px_counter && tile == 0 && tid == 0) atomicAdd(px_counter, (unsigned long long)P.H * (unsigned long long)P.W);

    // ---- 1. the tile's candidates, from its list: indices -> fresh headers (slic_assign_body, `listed`) ----------------------------
    int lk = -1;
    if (tid < l_n) lk = tl_k[(size_t)gtile * MAXC + tid];
    const unsigned myc4 = tl_fp[(size_t)gtile * NT + tid];
    if (tid < MAXC) r_acc[tid] = 0ull;
    if (lk >= 0) {
        const float4 *src = reinterpret_cast<const float4 *>(cent + (size_t)lk * RS);
        const float4 a = src[0], b = src[1];
        float4 *dh = reinterpret_cast<float4 *>(&r_hdr[tid][0]);
        dh[0] = a; dh[1] = b;
        r_k[tid] = lk;
    }
    const int nc = l_n;
    __syncthreads();
    RS_TICK(8)

    const int fy0 = ty0 + FB * wv;
    if (fy0 < P.H) {   // (a wave below the bottom edge only helps with the flush)
        const int fy1 = min(fy0 + FB, P.H);
        const int lane = lane_now();
        // ---- 2. prune the candidates of the wave's four footprints, one candidate per lane ----------------------------------------
        int cnt[SWEEP_TW / FB];
#pragma unroll
        for (int bxi = 0; bxi < SWEEP_TW / FB; ++bxi) {
            const int fx0 = tx0 + FB * bxi;
            cnt[bxi] = 0;
            if (fx0 >= P.W) continue;   // wave-uniform
            const int fx1 = min(fx0 + FB, P.W);
            const unsigned c = (myc4 >> (8 * bxi)) & 0xffu;
            unsigned lbb = 0xffffffffu, ubb = INF_BITS;
            bool hit = false;
            if (c != 0xffu) {
                const float4 h0 = *reinterpret_cast<const float4 *>(&r_hdr[c][0]);
                const float2 h1 = *reinterpret_cast<const float2 *>(&r_hdr[c][4]);
                const int y0 = __float_as_int(h0.z), y1 = __float_as_int(h0.w), x0 = __float_as_int(h1.x), x1 = __float_as_int(h1.y);
                if (y0 < fy1 && y1 > fy0 && x0 < fx1 && x1 > fx0) {   // the exact window of the fresh header
                    hit = true;
                    const float cy = h0.x, cx = h0.y;
                    const float ylo = (float)fy0, yhi = (float)(fy1 - 1), xlo = (float)fx0, xhi = (float)(fx1 - 1);
                    const float ry = (cy < ylo) ? ylo : ((cy > yhi) ? yhi : cy), rx = (cx < xlo) ? xlo : ((cx > xhi) ? xhi : cx);
                    const float tyn = cy - ry, txn = cx - rx;
                    lbb = __float_as_uint((tyn * tyn + txn * txn) * w);
                    if (y0 <= fy0 && y1 >= fy1 && x0 <= fx0 && x1 >= fx1) {
                        const float tyf = fmaxf(fabsf(cy - ylo), fabsf(cy - yhi)), txf = fmaxf(fabsf(cx - xlo), fabsf(cx - xhi));
                        ubb = __float_as_uint((tyf * tyf + txf * txf) * w);
                    }
                }
            }
            const unsigned bound = wave_umin(ubb);   // non-negative floats order like their bit patterns
            bool surv = hit && lbb <= bound;
            if (bound != INF_BITS) {
                // A = the covering candidate that attains the bound.  D_B - D_A is affine in (x, y) and D_A convex, so (T) at the four
                // corners of the footprint -- dt_B - dt_A at every corner above the margin of the largest dt_A -- proves as above that
                // B loses EVERY pixel of the footprint strictly to A, which exists on all of them: B is dropped (A itself stays: 0).
                const int la = (int)__builtin_ctzll(__ballot(ubb == bound));
                const int ca = __builtin_amdgcn_readlane((int)c, la);
                const float4 ha = *reinterpret_cast<const float4 *>(&r_hdr[ca][0]);
                const float4 hb = *reinterpret_cast<const float4 *>(&r_hdr[surv ? c : ca][0]);
                const float ylo = (float)fy0, yhi = (float)(fy1 - 1), xlo = (float)fx0, xhi = (float)(fx1 - 1);
                const float ay0 = (ha.x - ylo) * (ha.x - ylo), ay1 = (ha.x - yhi) * (ha.x - yhi), ax0 = (ha.y - xlo) * (ha.y - xlo), ax1 = (ha.y - xhi) * (ha.y - xhi);
                const float by0 = (hb.x - ylo) * (hb.x - ylo), by1 = (hb.x - yhi) * (hb.x - yhi), bx0 = (hb.y - xlo) * (hb.y - xlo), bx1 = (hb.y - xhi) * (hb.y - xhi);
                const float a00 = (ay0 + ax0) * w, a01 = (ay0 + ax1) * w, a10 = (ay1 + ax0) * w, a11 = (ay1 + ax1) * w;
                const float g = fminf(fminf((by0 + bx0) * w - a00, (by0 + bx1) * w - a01), fminf((by1 + bx0) * w - a10, (by1 + bx1) * w - a11));
                const float M = fmaxf(fmaxf(a00, a01), fmaxf(a10, a11));
                if (M < 3.0e38f && g > RUN_REL * M + RUN_ABS * w) surv = false;
            }
            const unsigned long long m = __ballot(surv);
            const unsigned pos = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (surv) r_surv[wv][bxi][pos] = (unsigned char)c;
            cnt[bxi] = __popcll(m);
        }
        wave_lds_sync();
        RS_TICK(9)

        // ---- 3. the lane's row segment: row fy0 + (lane & 15), columns [xa, xa + 16) of footprint lane >> 4 -----------------------
        const int seg = lane >> 4, y = fy0 + (lane & 15), xa = tx0 + FB * seg;
        const int mycnt = seg == 0 ? cnt[0] : (seg == 1 ? cnt[1] : (seg == 2 ? cnt[2] : cnt[3]));
        const unsigned char *sv = &r_surv[wv][seg][0];
        unsigned rowbits = 0u;   // bit i: pixel (y, xa + i) is inside the image and valid
        if (y < P.H && xa < P.W) {
            const int n = min(FB, P.W - xa);
            if ((long long)P.n_valid == (long long)P.H * (long long)P.W) {
                rowbits = 0xffffu >> (FB - n);
            } else {   // the packed mask: dword (y >> 2, x) holds the bytes of the rows 4 (y >> 2) .. + 3
                const unsigned *mp = mask4 + ((long long)P.m4_off + (long long)(y >> 2) * P.W + xa);
                const int sh = 8 * (y & 3);
#pragma unroll
                for (int i = 0; i < FB; ++i) {
                    const unsigned v = (i < n) ? mp[i] : 0u;
                    rowbits |= (unsigned)(((v >> sh) & 0xffu) != 0u) << i;
                }
            }
        }
        const float fy = (float)y;
        bool orphan = false;
        // a run [a, b] (absolute columns, inclusive) of slot k: its valid pixels go to the tile's accumulator in one LDS atomic
        auto add_run = [&](int k, int a, int b) {
            const unsigned bits = rowbits & (0xffffu >> (FB - 1 - (b - xa))) & (0xffffu << (a - xa)) & 0xffffu;
            if (!bits) return;
            if (k < 0) { orphan = true; return; }
            const unsigned m = __popc(bits);
            const unsigned sx = __popc(bits & 0xaaaau) + 2u * __popc(bits & 0xccccu) + 4u * __popc(bits & 0xf0f0u) + 8u * __popc(bits & 0xff00u) +
                                m * (unsigned)(xa - tx0);
            RS_COUNT(7, 1)
            atomicAdd(&r_acc[k], (unsigned long long)m | ((unsigned long long)(m * (unsigned)(y - ty0)) << 16) | ((unsigned long long)sx << 40));
        };
        // the reference's (d, k) minimum at one pixel, one candidate at a time in ascending k; d2: the smallest other distance (T)
        auto take = [](float d, bool in, int c, float &d1, float &d2, int &k1) {
            const bool t = in && d < d1;
            d2 = fminf(d2, t ? d1 : d);
            d1 = t ? d : d1;
            k1 = t ? c : k1;
        };
        const float abs_w = RUN_ABS * w;
        auto margin = [&](float d1a, float d2a, float d1b, float d2b) {
            const float M = fmaxf(d1a, d1b);
            return M < 3.0e38f && fminf(d2a - d1a, d2b - d1b) > RUN_REL * M + abs_w;
        };
        auto entry = [&](int a, int b) {
            return (unsigned)(a - xa) | ((unsigned)(b - xa) << 4) | ((unsigned)(lane & 15) << 8) | ((unsigned)seg << 12) | (rowbits << 16);
        };
        unsigned q0 = 0xffffffffu, q1 = 0xffffffffu;   // ranges of this lane that go to the pixel-by-pixel pass
        if (rowbits) {
            const int xl = xa + __builtin_ctz(rowbits), xr = xa + 31 - __builtin_clz(rowbits);   // first and last valid pixel
            const float fxl = (float)xl, fxr = (float)xr;
            float d1l = INFINITY, d2l = INFINITY, d1r = INFINITY, d2r = INFINITY;
            int k1l = -1, k1r = -1;
            for (int i = 0; i < mycnt; ++i) {
                const int c = sv[i];
                const float4 h0 = *reinterpret_cast<const float4 *>(&r_hdr[c][0]);
                const float2 h1 = *reinterpret_cast<const float2 *>(&r_hdr[c][4]);
                const int y0 = __float_as_int(h0.z), y1 = __float_as_int(h0.w), x0 = __float_as_int(h1.x), x1 = __float_as_int(h1.y);
                if ((unsigned)(y - y0) >= (unsigned)(y1 - y0)) continue;   // the candidate does not exist on this row
                const float ty = h0.x - fy, dy2 = ty * ty;
                const float tl = h0.y - fxl, tr = h0.y - fxr;
                take((dy2 + tl * tl) * w, xl >= x0 && xl < x1, c, d1l, d2l, k1l);
                take((dy2 + tr * tr) * w, xr >= x0 && xr < x1, c, d1r, d2r, k1r);
            }
            const int len = xr - xl + 1;
            RS_COUNT(1, 1) RS_COUNT(2, mycnt)
            if (k1l >= 0 && k1l == k1r && (len == 1 || margin(d1l, d2l, d1r, d2r))) {
                RS_COUNT(3, 1)
                add_run(k1l, xl, xr);
            } else if (len <= 2) {   // both pixels were evaluated
                add_run(k1l, xl, xl);
                if (len == 2) add_run(k1r, xr, xr);
            } else if (len >= 4 && k1l >= 0 && k1r >= 0 && k1l != k1r) {
                // one crossing expected: where the winner of the left end loses to the winner of the right end, from their
                // distances at both ends (the difference is affine in x).  Only a HINT for where to look: pixels m and m + 1
                // are evaluated, [xl, m - 1] and [m + 2, xr] are proven by (T) or queued.
                RS_COUNT(4, 1)
                const float4 ha = *reinterpret_cast<const float4 *>(&r_hdr[k1l][0]), hb = *reinterpret_cast<const float4 *>(&r_hdr[k1r][0]);
                const float tya = ha.x - fy, tyb = hb.x - fy, txa = ha.y - fxr, txb = hb.y - fxl;
                const float gl = (tyb * tyb + txb * txb) * w - d1l, gr = (tya * tya + txa * txa) * w - d1r;
                int m = xl + (int)(gl / (gl + gr) * (float)(len - 1));
                m = max(xl + 1, min(m, xr - 2));
                const int p0 = m - 1, p3 = m + 2;   // xl <= p0, p3 <= xr
                const float fp0 = (float)p0, fm = (float)m, fm1 = (float)(m + 1), fp3 = (float)p3;
                float e1p0 = INFINITY, e2p0 = INFINITY, e1p3 = INFINITY, e2p3 = INFINITY, e1m = INFINITY, e1m1 = INFINITY, dump = INFINITY;
                int kp0 = -1, kp3 = -1, km = -1, km1 = -1;
                for (int i = 0; i < mycnt; ++i) {
                    const int c = sv[i];
                    const float4 h0 = *reinterpret_cast<const float4 *>(&r_hdr[c][0]);
                    const float2 h1 = *reinterpret_cast<const float2 *>(&r_hdr[c][4]);
                    const int y0 = __float_as_int(h0.z), y1 = __float_as_int(h0.w), x0 = __float_as_int(h1.x), x1 = __float_as_int(h1.y);
                    if ((unsigned)(y - y0) >= (unsigned)(y1 - y0)) continue;
                    const float ty = h0.x - fy, dy2 = ty * ty;
                    const float t0 = h0.y - fp0, t1 = h0.y - fm, t2 = h0.y - fm1, t3 = h0.y - fp3;
                    take((dy2 + t0 * t0) * w, p0 >= x0 && p0 < x1, c, e1p0, e2p0, kp0);
                    take((dy2 + t1 * t1) * w, m >= x0 && m < x1, c, e1m, dump, km);
                    take((dy2 + t2 * t2) * w, m + 1 >= x0 && m + 1 < x1, c, e1m1, dump, km1);
                    take((dy2 + t3 * t3) * w, p3 >= x0 && p3 < x1, c, e1p3, e2p3, kp3);
                }
                const bool okl = kp0 == k1l && (p0 == xl || margin(d1l, d2l, e1p0, e2p0));
                const bool okr = kp3 == k1r && (p3 == xr || margin(e1p3, e2p3, d1r, d2r));
                bool mdone = false, m1done = false;
                if (okl) { mdone = km == k1l; add_run(k1l, xl, mdone ? m : p0); } else q0 = entry(xl, p0);
                if (okr) { m1done = km1 == k1r; add_run(k1r, m1done ? m + 1 : p3, xr); } else q1 = entry(p3, xr);
                if (!mdone) add_run(km, m, m);
                if (!m1done) add_run(km1, m + 1, m + 1);
            } else {
                q0 = entry(xl, xr);
            }
        }
        // ---- 4. what was not proven: pixel by pixel, sixteen lanes per queued range -------------------------------------------------
        int qn = 0;
        {
            const unsigned long long m0 = __ballot(q0 != 0xffffffffu);
            if (q0 != 0xffffffffu) r_q[wv][__builtin_amdgcn_mbcnt_hi((unsigned)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m0, 0u))] = q0;
            qn = __popcll(m0);
            const unsigned long long m1 = __ballot(q1 != 0xffffffffu);
            if (q1 != 0xffffffffu) r_q[wv][qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m1, 0u))] = q1;
            qn += __popcll(m1);
        }
        wave_lds_sync();
        RS_TICK(10)
        RS_COUNT(5, lane == 0 ? qn : 0)
        for (int base = 0; base < qn; base += 4) {   // wave-uniform
            const int ei = base + (lane >> 4);
            if (ei >= qn) continue;
            const unsigned e = r_q[wv][ei];
            const int xrel = (int)(e & 15u) + (lane & 15);
            if (xrel > (int)((e >> 4) & 15u) || !((e >> (16 + xrel)) & 1u)) continue;   // outside the range, or not a valid pixel
            RS_COUNT(6, 1)
            const int qs = (int)((e >> 12) & 3u), qy = fy0 + (int)((e >> 8) & 15u), qx = tx0 + FB * qs + xrel;
            const int qcnt = qs == 0 ? cnt[0] : (qs == 1 ? cnt[1] : (qs == 2 ? cnt[2] : cnt[3]));
            const unsigned char *qv = &r_surv[wv][qs][0];
            const float fqy = (float)qy, fqx = (float)qx;
            float best = INFINITY;
            int bk = -1;
            for (int i = 0; i < qcnt; ++i) {
                const int c = qv[i];
                const float4 h0 = *reinterpret_cast<const float4 *>(&r_hdr[c][0]);
                const float2 h1 = *reinterpret_cast<const float2 *>(&r_hdr[c][4]);
                const int y0 = __float_as_int(h0.z), y1 = __float_as_int(h0.w), x0 = __float_as_int(h1.x), x1 = __float_as_int(h1.y);
                if (!(qy >= y0 && qy < y1 && qx >= x0 && qx < x1)) continue;
                const float ty = h0.x - fqy, tx = h0.y - fqx;
                const float d = (ty * ty + tx * tx) * w;
                if (d < best) { best = d; bk = c; }   // ascending k: a tie stays with the lowest
            }
            if (bk < 0) orphan = true;
            else atomicAdd(&r_acc[bk], 1ull | ((unsigned long long)(unsigned)(qy - ty0) << 16) | ((unsigned long long)(unsigned)(qx - tx0) << 40));
        }
        // a valid pixel that no window reached keeps the label of the sweep before, which was not stored: the host repeats the batch
        if (__ballot(orphan) && lane == 0) *orphan_flag = 1;
        RS_TICK(11)
        RS_FLUSH
    }
    __syncthreads();
    // ---- 5. LDS accumulators -> global records (n, sum_y, sum_x; the colour words of a spatial-only sweep are never read) --------
    const int tid_e = wv * 64 + lane_now();
    for (int i = tid_e; i < nc * 3; i += NT) {
        const int slot = i / 3, q = i - slot * 3;
        const unsigned long long pw = r_acc[slot];
        const unsigned long long n = pw & 0xffffull;
        if (n == 0ull) continue;
        const unsigned long long v = q == 0 ? n : (q == 1 ? ((pw >> 16) & 0xffffffull) + n * (unsigned long long)ty0 : (pw >> 40) + n * (unsigned long long)tx0);
        atomicAdd(&acc[(size_t)r_k[slot] * RQ + CP + q], v);
    }
    RS_TICK(12)
}

// the pre-pass sweeps that fold no colours and store no labels (and keep no fixed-point cache): runs where the tile has a list
template <int CP>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(LEAN_WAVES, LEAN_WAVES))) void slic_spatial_kernel(OBIA_ASSIGN_PARAMS, const int *__restrict__ act_tiles) {
    // (the tile of this workgroup and its list state: as in slic_assign_body)
    constexpr int XG = OBIA_XCD_GROUP;
    const int gslot = tile_base + (((int)(blockIdx.x >> 3) / XG) * 8 + (int)(blockIdx.x & 7)) * XG + (int)(blockIdx.x >> 3) % XG;
    if (gslot >= total_tiles_all) return;
    const int gtile = act_tiles ? act_tiles[gslot] : gslot;
    const int l_n = tl_meta[2 * (size_t)gtile], l_bw = tl_meta[2 * (size_t)gtile + 1], l_req = tl_req[gtile];
    const int prob_i = tiles_per_prob > 0 ? gtile / tiles_per_prob : tile_prob[gtile];
    const SlicProblem P = probs[prob_i];
    const bool listed = l_n >= 0 && l_bw >= 0 && l_req <= (l_bw & 0xffff);
    if (listed && accumulate && !store_labels && !P.direct && P.spatial_w >= RUN_W_LO && P.spatial_w <= RUN_W_HI)   // workgroup-uniform
        slic_spatial_tile<CP>(P, gtile, gtile - P.tile_off, l_n, mask4, cent, acc, RQ, px_counter, orphan_flag, tl_k, tl_fp);
    else
        slic_assign_body<CP, true, true, false, false, true, false>(OBIA_ASSIGN_ARGS, act_tiles);
}
