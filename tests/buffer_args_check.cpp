// buffer_args_check.cpp -- the argument checks of the entry layer (obia_amd/csrc/buffer_args.hpp) against the expressions they
// replaced.  A program of its own, built and run by tests/test_buffer_args_cpu.py with the host compiler and -fsanitize=address,undefined.
//
// The expected verdict is always formed the old way: misaligned() and shared_start() below are the functions common.hpp had, and the
// old_* functions are the conditions the five entry points had.  The pointers are made from integers; nothing is read through them.
// With -DTRY_VOID or -DTRY_CONST_OUT the program must NOT compile (the test asserts that).
#include <cinttypes>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../obia_amd/csrc/buffer_args.hpp"

static char g_error[512];
namespace obia {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace obia
using obia::Buffers;
using obia::OPTIONAL;
using obia::Refusal;

// ---- what common.hpp had, word for word ---------------------------------------------------------------------------------------------
inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
template <typename... P> bool shared_start(int n_out, P... ps) {
    const void *v[] = {static_cast<const void *>(ps)...};
    const int m = (int)sizeof...(ps);
    for (int i = 0; i < n_out; ++i)
        for (int j = i + 1; j < m; ++j)
            if (v[i] && v[i] == v[j]) return true;
    return false;
}

static long long g_checks = 0;
static int g_failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        ++g_checks;                                                                     \
        if (!(cond) && ++g_failures <= 20) printf("line %d: %s\n", __LINE__, #cond);    \
    } while (0)

constexpr uintptr_t BASE = 0x10000;   // a multiple of 16
template <typename T> T *at(uintptr_t v) { return reinterpret_cast<T *>(v); }

// ---- (a) alignment comes from the pointee, (b) needed / optional / needed if n > 0 -------------------------------------------------
template <typename T> void alignment_and_null() {
    for (uintptr_t r = 0; r < 16; ++r) {
        T *p = at<T>(BASE + r);
        const bool want = r % alignof(T) != 0;
        CHECK(want == misaligned(p, alignof(T)));
        CHECK(Buffers().out(p).bad() == want);
        CHECK(Buffers().in(p).bad() == want);
        CHECK(Buffers().lone(p).bad() == want);
        CHECK(Buffers().out<16>(p).bad() == (r != 0));
        CHECK(Buffers().in<16>(p).bad() == (r != 0));
        CHECK(Buffers().lone<16>(p).bad() == (r != 0) && misaligned(p, 16) == (r != 0));
        CHECK(Buffers().lone<1>(p).bad() == false);              // the explicit form may also ask for less: a site keeps what it had
    }
    T *null = nullptr, *p = at<T>(BASE);
    CHECK(Buffers().out(null).bad() && Buffers().in(null).bad() && Buffers().lone(null).bad());
    CHECK(!Buffers().out(null, OPTIONAL).bad() && !Buffers().in(null, OPTIONAL).bad() && !Buffers().lone(null, OPTIONAL).bad());
    CHECK(!Buffers().out<16>(null, OPTIONAL).bad());
    for (long long n = 0; n < 2; ++n) {
        CHECK(Buffers().in(null, n > 0).bad() == (n > 0));
        CHECK(Buffers().out(null, n > 0).bad() == (n > 0));
        CHECK(!Buffers().in(p, n > 0).bad());
    }
}

// ---- (c) overlap ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename U> void overlap() {
    T *o = at<T>(BASE), *o2 = at<T>(BASE + 64), *tnull = nullptr;
    const U *same = at<const U>(BASE), *other = at<const U>(BASE + 32), *unull = nullptr;
    CHECK(Buffers().out(o).in(same).bad() && shared_start(1, o, same));
    CHECK(Buffers().in(same).out(o).bad());                      // whichever is listed first
    CHECK(Buffers().out(o).out(at<T>(BASE)).bad() && shared_start(2, o, at<T>(BASE)));
    CHECK(Buffers().out(o2).in(other).in(same).out(o).bad() && shared_start(2, o2, o, other, same));
    CHECK(!Buffers().out(o).in(other).bad() && !shared_start(1, o, other));
    CHECK(!Buffers().out(o2).in(same).in(at<const U>(BASE)).bad() && !shared_start(1, o2, same, at<const U>(BASE)));   // two inputs may share
    CHECK(!Buffers().out(o).lone(same).bad());                   // a lone buffer is compared with nothing
    CHECK(!Buffers().lone(same).out(o).bad());
    CHECK(!Buffers().out(tnull, OPTIONAL).in(unull, OPTIONAL).out(at<T>(0), OPTIONAL).bad() && !shared_start(2, tnull, tnull, unull));   // a null never overlaps
    CHECK(Buffers().out(o).in(at<const U>(BASE + 1)).bad() == (alignof(U) > 1));    // starts, not ranges: one byte on is another start, and only its alignment can refuse it
}

// ---- (d) capacity: fourteen buffers are accepted, a fifteenth is REFUSED (at run time: bad()) --------------------------------------
void capacity() {
    Buffers b;
    for (int i = 0; i < Buffers::CAPACITY; ++i) {
        if (i % 3 == 0) b.out(at<double>(BASE + 16 * i));
        else b.in(at<const int32_t>(BASE + 16 * i));
        CHECK(!b.bad());
    }
    CHECK(Buffers::CAPACITY == 14);
    b.lone(at<const float>(BASE + 16 * 40)).lone(at<const float>(BASE + 16 * 41));
    CHECK(!b.bad());                                             // lone buffers take no room
    b.in(at<const float>(BASE + 16 * 50));
    CHECK(b.bad());
}

// ---- (e) five entry points: the condition each had, and the listing each has now ----------------------------------------------------
struct Args { uintptr_t v[16]; long long n1, n2; };

// boxes.hip, obia_boxes_pair_write_dev
#define PAIR_WRITE_ARGS const int32_t *labels, const double *boxes, const int64_t *offset, const int32_t *passes, int32_t *box_out, \
                        int32_t *segment_out, double *area_out, int32_t *meets_out
bool old_pair_write(PAIR_WRITE_ARGS) {
    return !labels || !boxes || !offset || !passes || !box_out || !segment_out || !area_out || !meets_out || misaligned(labels, 4) ||
           misaligned(boxes, 8) || misaligned(offset, 8) || misaligned(passes, 4) || misaligned(box_out, 4) || misaligned(segment_out, 4) ||
           misaligned(area_out, 8) || misaligned(meets_out, 4) ||
           shared_start(4, box_out, segment_out, area_out, meets_out, labels, boxes, offset, passes);
}
bool new_pair_write(PAIR_WRITE_ARGS) {
    return Buffers().out(box_out).out(segment_out).out(area_out).out(meets_out).in(labels).in(boxes).in(offset).in(passes).bad();
}

// points.hip, obia_points_segment_columns_dev
#define COLUMNS_ARGS const uint32_t *profile, const uint32_t *top, const uint32_t *n_int, const uint64_t *s1, const uint64_t *s2,   \
                     int64_t *n_points, double *ch, double *pai, double *fhd, double *mean_intensity, double *variance_intensity, \
                     double *pad
bool old_columns(COLUMNS_ARGS) {
    return !profile || !top || !n_int || !s1 || !s2 || !n_points || !ch || !pai || !fhd || !mean_intensity || !variance_intensity ||
           misaligned(profile, 4) || misaligned(top, 4) || misaligned(n_int, 4) || misaligned(s1, 8) || misaligned(s2, 8) || misaligned(n_points, 8) ||
           misaligned(ch, 8) || misaligned(pai, 8) || misaligned(fhd, 8) || misaligned(mean_intensity, 8) || misaligned(variance_intensity, 8) ||
           misaligned(pad, 8) ||
           shared_start(7, n_points, ch, pai, fhd, mean_intensity, variance_intensity, pad, profile, top, n_int, s1, s2);
}
bool new_columns(COLUMNS_ARGS) {
    Buffers b;
    b.in(profile).in(top).in(n_int).in(s1).in(s2);
    return b.out(n_points).out(ch).out(pai).out(fhd).out(mean_intensity).out(variance_intensity).out(pad, OPTIONAL).bad();
}

// merging.hip, obia_merge_pairs_dev
bool old_csr_missing(const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t N, int64_t nnz) {
    return (N > 0 && !indptr) || (nnz > 0 && (!neighbor || !border)) || misaligned(indptr, 8) || misaligned(neighbor, 4) || misaligned(border, 8);
}
bool old_tables_missing(int32_t N, const int64_t *area, const double *mean, const double *m2, const int64_t *perimeter, const int32_t *box) {
    return (N > 0 && (!area || !mean || !m2 || !perimeter || !box)) || misaligned(area, 8) || misaligned(mean, 8) || misaligned(m2, 8) ||
           misaligned(perimeter, 8) || misaligned(box, 4);
}
Buffers &list_csr(Buffers &b, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t N, int64_t nnz) {
    return b.in(indptr, N > 0).in(neighbor, nnz > 0).in(border, nnz > 0);
}
Buffers &list_tables(Buffers &b, int32_t N, const int64_t *area, const double *mean, const double *m2, const int64_t *perimeter, const int32_t *box) {
    return b.in(area, N > 0).in(mean, N > 0).in(m2, N > 0).in(perimeter, N > 0).in(box, N > 0);
}
Buffers &list_tables_out(Buffers &b, int32_t N, int64_t *area, double *mean, double *m2, int64_t *perimeter, int32_t *box) {
    return b.out(area, N > 0).out(mean, N > 0).out(m2, N > 0).out(perimeter, N > 0).out(box, N > 0);
}
#define PAIRS_ARGS const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels, int64_t nnz,             \
                   const int32_t *partner, const int64_t *area, const double *mean, const double *m2, const int64_t *perimeter,    \
                   const int32_t *box, int64_t *area_out, double *mean_out, double *m2_out, int64_t *perimeter_out, int32_t *box_out
bool old_pairs(PAIRS_ARGS) {
    return old_csr_missing(indptr, neighbor, border, n_labels, nnz) || old_tables_missing(n_labels, area, mean, m2, perimeter, box) ||
           old_tables_missing(n_labels, area_out, mean_out, m2_out, perimeter_out, box_out) || (n_labels > 0 && !partner) || misaligned(partner, 4) ||
           shared_start(5, area_out, mean_out, m2_out, perimeter_out, box_out, indptr, neighbor, border, partner, area, mean, m2, perimeter, box);
}
bool new_pairs(PAIRS_ARGS) {
    Buffers b;
    list_csr(b, indptr, neighbor, border, n_labels, nnz).in(partner, n_labels > 0);
    list_tables(b, n_labels, area, mean, m2, perimeter, box);
    return list_tables_out(b, n_labels, area_out, mean_out, m2_out, perimeter_out, box_out).bad();
}

// ground.hip, obia_ground_query_dev: the rule that z and hag come together stands outside the checker
#define QUERY_ARGS const double *gx, const double *gy, const double *gz, const int32_t *gidx, const int32_t *cell_start, const double *x, \
                   const double *y, const double *z, int64_t n, double *zg, float *hag, uint8_t *m
bool old_query(QUERY_ARGS) {
    return !gx || !gy || !gz || !gidx || !cell_start || !zg || (n > 0 && (!x || !y)) || (z == nullptr) != (hag == nullptr) || misaligned(gx, 8) ||
           misaligned(gy, 8) || misaligned(gz, 8) || misaligned(gidx, 4) || misaligned(cell_start, 4) || misaligned(x, 8) || misaligned(y, 8) ||
           misaligned(z, 8) || misaligned(zg, 8) || misaligned(hag, 4) || shared_start(3, zg, hag, m, gx, gy, gz, gidx, cell_start, x, y, z);
}
bool new_query(QUERY_ARGS) {
    Buffers b;
    b.in(gx).in(gy).in(gz).in(gidx).in(cell_start).in(x, n > 0).in(y, n > 0).in(z, OPTIONAL);
    return (z == nullptr) != (hag == nullptr) || b.out(zg).out(hag, OPTIONAL).out(m, OPTIONAL).bad();
}

// sharpness.hip, obia_sharp_box_dev
bool old_sharp_box(const float *plane, float *work, float *out) {
    return !plane || !work || !out || plane == out || plane == work || work == out || ((uintptr_t)plane & 3) || ((uintptr_t)work & 3) ||
           ((uintptr_t)out & 3);
}
bool new_sharp_box(const float *plane, float *work, float *out) { return Buffers().out(work).out(out).in(plane).bad(); }

struct Site {
    const char *name;
    int nargs, out0, nvary;                                      // the first nvary arguments of `order` take every state, the rest are valid
    int size[16], order[16];
    bool (*old_way)(const Args &), (*new_way)(const Args &);
};

// the states of an argument: null, aligned, one element on, one byte on, where output 0 starts
uintptr_t value_of(const Site &s, int i, int state, uintptr_t out0) {
    const uintptr_t home = BASE + 0x1000 * (uintptr_t)(i + 1);
    switch (state) {
        case 0: return 0;
        case 1: return home;
        case 2: return home + (uintptr_t)s.size[i];
        case 3: return home + 1;
        default: return i == s.out0 ? BASE + 0x1000 * (uintptr_t)((i + 1) % s.nargs + 1) : out0;   // output 0 itself: where its neighbour lives
    }
}
void sweep(const Site &s, long long n1, long long n2) {
    int state[16];
    for (int i = 0; i < s.nargs; ++i) state[i] = 1;
    long long cases = 1, refused = 0;
    for (int k = 0; k < s.nvary; ++k) cases *= 5;
    for (long long c = 0; c < cases; ++c) {
        long long rest = c;
        for (int k = 0; k < s.nvary; ++k, rest /= 5) state[s.order[k]] = (int)(rest % 5);
        Args a{};
        a.n1 = n1; a.n2 = n2;
        const uintptr_t out0 = value_of(s, s.out0, state[s.out0], 0);
        for (int i = 0; i < s.nargs; ++i) a.v[i] = i == s.out0 ? out0 : value_of(s, i, state[i], out0);
        const bool want = s.old_way(a), got = s.new_way(a);
        refused += want;
        ++g_checks;
        if (want != got && ++g_failures <= 20) {
            printf("%s (n1 %lld, n2 %lld): the condition says %d, the listing %d, at states", s.name, n1, n2, (int)want, (int)got);
            for (int i = 0; i < s.nargs; ++i) printf(" %d", state[i]);
            printf("\n");
        }
    }
    printf("%-28s n1 %lld n2 %lld: %lld cases, %lld refused\n", s.name, n1, n2, cases, refused);
    CHECK(refused > 0 && refused < cases);
}

#define P(T, i) at<T>(a.v[i])
const Site SITES[] = {
    {"boxes: pair write", 8, 4, 8, {4, 8, 8, 4, 4, 4, 8, 4}, {0, 1, 2, 3, 4, 5, 6, 7},
     [](const Args &a) { return old_pair_write(P(const int32_t, 0), P(const double, 1), P(const int64_t, 2), P(const int32_t, 3), P(int32_t, 4), P(int32_t, 5), P(double, 6), P(int32_t, 7)); },
     [](const Args &a) { return new_pair_write(P(const int32_t, 0), P(const double, 1), P(const int64_t, 2), P(const int32_t, 3), P(int32_t, 4), P(int32_t, 5), P(double, 6), P(int32_t, 7)); }},
    {"points: segment columns", 12, 5, 8, {4, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8}, {5, 0, 3, 6, 11, 1, 4, 10, 2, 7, 8, 9},
     [](const Args &a) { return old_columns(P(const uint32_t, 0), P(const uint32_t, 1), P(const uint32_t, 2), P(const uint64_t, 3), P(const uint64_t, 4), P(int64_t, 5), P(double, 6), P(double, 7), P(double, 8), P(double, 9), P(double, 10), P(double, 11)); },
     [](const Args &a) { return new_columns(P(const uint32_t, 0), P(const uint32_t, 1), P(const uint32_t, 2), P(const uint64_t, 3), P(const uint64_t, 4), P(int64_t, 5), P(double, 6), P(double, 7), P(double, 8), P(double, 9), P(double, 10), P(double, 11)); }},
    {"merging: pairs", 14, 9, 7, {8, 4, 8, 4, 8, 8, 8, 8, 4, 8, 8, 8, 8, 4}, {9, 0, 1, 3, 4, 8, 13, 2, 5, 6, 7, 10, 11, 12},
     [](const Args &a) { return old_pairs(P(const int64_t, 0), P(const int32_t, 1), P(const int64_t, 2), (int32_t)a.n1, a.n2, P(const int32_t, 3), P(const int64_t, 4), P(const double, 5), P(const double, 6), P(const int64_t, 7), P(const int32_t, 8), P(int64_t, 9), P(double, 10), P(double, 11), P(int64_t, 12), P(int32_t, 13)); },
     [](const Args &a) { return new_pairs(P(const int64_t, 0), P(const int32_t, 1), P(const int64_t, 2), (int32_t)a.n1, a.n2, P(const int32_t, 3), P(const int64_t, 4), P(const double, 5), P(const double, 6), P(const int64_t, 7), P(const int32_t, 8), P(int64_t, 9), P(double, 10), P(double, 11), P(int64_t, 12), P(int32_t, 13)); }},
    {"ground: query", 11, 8, 8, {8, 8, 8, 4, 4, 8, 8, 8, 8, 4, 1}, {8, 9, 10, 7, 0, 3, 5, 6, 1, 2, 4},
     [](const Args &a) { return old_query(P(const double, 0), P(const double, 1), P(const double, 2), P(const int32_t, 3), P(const int32_t, 4), P(const double, 5), P(const double, 6), P(const double, 7), a.n1, P(double, 8), P(float, 9), P(uint8_t, 10)); },
     [](const Args &a) { return new_query(P(const double, 0), P(const double, 1), P(const double, 2), P(const int32_t, 3), P(const int32_t, 4), P(const double, 5), P(const double, 6), P(const double, 7), a.n1, P(double, 8), P(float, 9), P(uint8_t, 10)); }},
    {"sharpness: box", 3, 2, 3, {4, 4, 4}, {0, 1, 2},
     [](const Args &a) { return old_sharp_box(P(const float, 0), P(float, 1), P(float, 2)); },
     [](const Args &a) { return new_sharp_box(P(const float, 0), P(float, 1), P(float, 2)); }},
};

// ---- (f) the refusals: the text and the code each file's helper gave ----------------------------------------------------------------
void expect(int rc, int code, const char *fmt, ...) {
    char want[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(want, sizeof want, fmt, ap);
    va_end(ap);
    ++g_checks;
    if ((rc != code || strcmp(want, g_error) != 0) && ++g_failures <= 20) printf("refusal: %d \"%s\", expected %d \"%s\"\n", rc, g_error, code, want);
    g_error[0] = 0;
}
void quiet(int rc) {
    CHECK(rc == OBIA_OK && g_error[0] == 0);
}
void refusals() {
    const long long big = (long long)INT_MAX + 1;
    // bad_buffers: seed_table, boxes, points, ground, groundfilter, adjacency, merging (and the text shapes.hip spelt out)
    expect(Refusal{"boxes", "pair write"}.buffers(), OBIA_E_INVALID, "boxes: %s: bad arguments (null, misaligned or overlapping buffers)", "pair write");
    expect(Refusal{"seed table", "stage 1"}.buffers(), OBIA_E_INVALID, "seed table: %s: bad arguments (null, misaligned or overlapping buffers)", "stage 1");
    expect(Refusal{"shapes", "sums"}.buffers(), OBIA_E_INVALID, "shapes: sums: bad arguments (null, misaligned or overlapping buffers)");
    // check_n from 1 (seed_table, boxes): OBIA_E_INVALID on either side
    const Refusal nms{"boxes", "nms"};
    expect(nms.n(0), OBIA_E_INVALID, "boxes: %s: n must be in 1 .. 2^31 - 1, got %lld", "nms", 0ll);
    expect(nms.n(big), OBIA_E_INVALID, "boxes: %s: n must be in 1 .. 2^31 - 1, got %lld", "nms", big);
    expect(Refusal{"seed table", "cells"}.n(-3), OBIA_E_INVALID, "seed table: %s: n must be in 1 .. 2^31 - 1, got %lld", "cells", -3ll);
    quiet(nms.n(1));
    quiet(nms.n(INT_MAX));
    // check_n from 0 (ground, groundfilter, the head of points' check_cloud): above 2^31 - 1 is OBIA_E_UNSUPPORTED
    const Refusal query{"ground", "query"};
    expect(query.n_or_none(-1), OBIA_E_INVALID, "ground: %s: n must not be negative, got %lld", "query", -1ll);
    expect(query.n_or_none(big), OBIA_E_UNSUPPORTED, "ground: %s: n must be below 2^31 per call, got %lld", "query", big);
    expect(Refusal{"points", "rasters"}.n_or_none(big), OBIA_E_UNSUPPORTED, "points: %s: n must be below 2^31 per call, got %lld", "rasters", big);
    expect(Refusal{"groundfilter", "classify"}.n_or_none(-7), OBIA_E_INVALID, "groundfilter: %s: n must not be negative, got %lld", "classify", -7ll);
    quiet(query.n_or_none(0));
    quiet(query.n_or_none(INT_MAX));
    // check_raster: points (H and W alone), adjacency and groundfilter (H * W below 2^31), boxes (with n_labels)
    const Refusal finish{"points", "rasters finish"}, filter{"groundfilter", "filter"}, tile{"adjacency", "tile count"}, assign{"boxes", "assign"};
    expect(finish.raster(0, 5), OBIA_E_INVALID, "points: %s: H and W must be positive, got %d x %d", "rasters finish", 0, 5);
    expect(finish.raster(5, -1), OBIA_E_INVALID, "points: %s: H and W must be positive, got %d x %d", "rasters finish", 5, -1);
    quiet(finish.raster(65536, 32768));
    expect(filter.raster_below_2_31(0, 5), OBIA_E_INVALID, "groundfilter: %s: H and W must be positive, got %d x %d", "filter", 0, 5);
    expect(filter.raster_below_2_31(65536, 32768), OBIA_E_UNSUPPORTED, "groundfilter: %s: H * W must be below 2^31, got %d x %d", "filter", 65536, 32768);
    expect(tile.raster_below_2_31(32768, 65536), OBIA_E_UNSUPPORTED, "adjacency: %s: H * W must be below 2^31, got %d x %d", "tile count", 32768, 65536);
    quiet(tile.raster_below_2_31(INT_MAX, 1));
    expect(assign.raster(5, 0, 3), OBIA_E_INVALID, "boxes: %s: H and W must be positive, got %d x %d", "assign", 5, 0);
    expect(assign.raster(5, 5, -1), OBIA_E_INVALID, "boxes: %s: n_labels must be in 0 .. 2^31 - 2, got %d", "assign", -1);
    expect(assign.raster(5, 5, INT_MAX), OBIA_E_INVALID, "boxes: %s: n_labels must be in 0 .. 2^31 - 2, got %d", "assign", INT_MAX);
    quiet(assign.raster(65536, 32768, INT_MAX - 1));
    // check_labels and check_count (adjacency, merging)
    const Refusal cost{"merging", "cost"}, d2{"adjacency", "edge d2"};
    expect(cost.labels(-1), OBIA_E_INVALID, "merging: %s: n_labels must be in 0 .. 2^31 - 3, got %d", "cost", -1);
    expect(d2.labels(INT_MAX - 1), OBIA_E_INVALID, "adjacency: %s: n_labels must be in 0 .. 2^31 - 3, got %d", "edge d2", INT_MAX - 1);
    quiet(d2.labels(INT_MAX - 2));
    quiet(cost.labels(0));
    expect(d2.count("F", 0, 1), OBIA_E_INVALID, "adjacency: %s: %s must be at least %lld, got %lld", "edge d2", "F", 1ll, 0ll);
    expect(cost.count("nnz", -1, 0), OBIA_E_INVALID, "merging: %s: %s must be at least %lld, got %lld", "cost", "nnz", 0ll, -1ll);
    expect(cost.count("n_labels * F", big, 0), OBIA_E_UNSUPPORTED, "merging: %s: %s must be below 2^31, got %lld", "cost", "n_labels * F", big);
    expect(d2.count("nnz", big, 0), OBIA_E_UNSUPPORTED, "adjacency: %s: %s must be below 2^31, got %lld", "edge d2", "nnz", big);
    quiet(d2.count("nnz", 0, 0));
    quiet(cost.count("F", INT_MAX, 1));
}

#if defined(TRY_VOID)
bool must_not_compile(const void *p) { return Buffers().in(p).bad(); }               // a pointer to void states its alignment: in<16>(p)
#endif
#if defined(TRY_CONST_OUT)
bool must_not_compile(const float *p) { return Buffers().out(p).bad(); }             // nothing is written through a pointer to const
#endif

int main() {
    alignment_and_null<uint8_t>();
    alignment_and_null<uint16_t>();
    alignment_and_null<int32_t>();
    alignment_and_null<float>();
    alignment_and_null<int64_t>();
    alignment_and_null<double>();
    CHECK(!Buffers().in<8>(static_cast<const void *>(at<char>(BASE + 8))).bad() && Buffers().in<16>(static_cast<const void *>(at<char>(BASE + 8))).bad());
    overlap<int32_t, float>();
    overlap<double, int64_t>();
    overlap<uint8_t, uint8_t>();
    overlap<uint16_t, double>();
    capacity();
    for (const Site &s : SITES) {
        sweep(s, 3, 5);
        sweep(s, 0, 0);
    }
    refusals();
    printf("%lld checks, %d failed\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
