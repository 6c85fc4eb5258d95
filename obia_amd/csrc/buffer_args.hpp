// buffer_args.hpp -- the argument checks of an extern "C" function, the fourth piece of the entry layer (common.hpp): Buffers, through
// which an entry point lists each of its device buffers ONCE and learns whether one is null, misaligned or overlapping; and Refusal,
// the messages and status codes with which every operator turns a call down.  Host code only: nothing of HIP is needed here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/obia_hip.h"

namespace obia {

void set_error(const char *fmt, ...);

// The alignment a buffer needs is that of the type its parameter points to.  A pointer to void has none: such a buffer states its
// alignment (out<16>(p)), and so does one that needs more than its type does.
template <typename T> struct Pointee { static constexpr size_t align = alignof(T); };
template <> struct Pointee<void>;
template <> struct Pointee<const void>;

constexpr bool OPTIONAL = false;   // second argument of out() / in() / lone(): the buffer may be null.  Or a condition: in(x, n > 0)

// out(p): a buffer the call writes; it must not START where another out() or an in() starts (starts are compared, not ranges).
// in(p): a buffer the call reads.  lone(p): a buffer that is judged on its own -- null and alignment -- and compared with nothing:
// for the entry points that have always compared only some pairs.  A null buffer is refused if it is needed, and is otherwise aligned
// and overlaps nothing.  Up to CAPACITY out() and in() buffers; one more makes the call bad().
class Buffers {
  public:
    static constexpr int CAPACITY = 14;
    template <size_t A = 0, typename T> Buffers &out(T *p, bool needed = true) { return add(p, align_of<A, T>(), needed, OUT); }
    template <size_t A = 0, typename T> Buffers &out(const T *p, bool needed = true) = delete;   // nothing is written through it
    template <size_t A = 0, typename T> Buffers &in(const T *p, bool needed = true) { return add(p, align_of<A, T>(), needed, IN); }
    template <size_t A = 0, typename T> Buffers &lone(const T *p, bool needed = true) { return add(p, align_of<A, T>(), needed, LONE); }
    bool bad() const { return bad_; }

  private:
    enum Role { OUT, IN, LONE };
    template <size_t A, typename T> static constexpr size_t align_of() {
        if constexpr (A != 0) return A;
        else return Pointee<T>::align;
    }
    Buffers &add(const void *p, size_t align, bool needed, Role role) {
        if (!p) {
            bad_ |= needed;
            return *this;
        }
        if (((uintptr_t)p & (align - 1)) != 0) bad_ = true;
        if (role == LONE) return *this;
        for (int i = 0; i < n_; ++i)
            if (start_[i] == p && (role == OUT || is_out_[i])) bad_ = true;
        if (n_ == CAPACITY) {
            bad_ = true;
            return *this;
        }
        start_[n_] = p;
        is_out_[n_++] = role == OUT;
        return *this;
    }
    const void *start_[CAPACITY];
    bool is_out_[CAPACITY];
    int n_ = 0;
    bool bad_ = false;
};

// What an operator answers to a call it turns down: Refusal{"boxes", "pair write"}.buffers().  Every member that judges a value
// returns OBIA_OK when there is nothing to refuse.
struct Refusal {
    const char *module, *what;

    int buffers() const {
        set_error("%s: %s: bad arguments (null, misaligned or overlapping buffers)", module, what);
        return OBIA_E_INVALID;
    }
    // n of a call that needs an element: 1 .. 2^31 - 1
    int n(int64_t n) const {
        if (n < 1 || n > (int64_t)INT32_MAX) { set_error("%s: %s: n must be in 1 .. 2^31 - 1, got %lld", module, what, (long long)n); return OBIA_E_INVALID; }
        return OBIA_OK;
    }
    // n of a call that may be empty: 0 .. 2^31 - 1, more is valid and not implemented
    int n_or_none(int64_t n) const {
        if (n < 0) { set_error("%s: %s: n must not be negative, got %lld", module, what, (long long)n); return OBIA_E_INVALID; }
        if (n > (int64_t)INT32_MAX) { set_error("%s: %s: n must be below 2^31 per call, got %lld", module, what, (long long)n); return OBIA_E_UNSUPPORTED; }
        return OBIA_OK;
    }
    int raster(int H, int W) const {
        if (H <= 0 || W <= 0) { set_error("%s: %s: H and W must be positive, got %d x %d", module, what, H, W); return OBIA_E_INVALID; }
        return OBIA_OK;
    }
    // ... whose pixels are counted in an int
    int raster_below_2_31(int H, int W) const {
        if (int rc = raster(H, W)) return rc;
        if ((long long)H * W > (long long)INT32_MAX) { set_error("%s: %s: H * W must be below 2^31, got %d x %d", module, what, H, W); return OBIA_E_UNSUPPORTED; }
        return OBIA_OK;
    }
    // ... with labels 0 .. n_labels, the largest int kept free (boxes.hip)
    int raster(int H, int W, int32_t n_labels) const {
        if (int rc = raster(H, W)) return rc;
        if (n_labels < 0 || n_labels == INT32_MAX) { set_error("%s: %s: n_labels must be in 0 .. 2^31 - 2, got %d", module, what, n_labels); return OBIA_E_INVALID; }
        return OBIA_OK;
    }
    int labels(int32_t n_labels) const {
        if (n_labels < 0 || n_labels > INT32_MAX - 2) { set_error("%s: %s: n_labels must be in 0 .. 2^31 - 3, got %d", module, what, n_labels); return OBIA_E_INVALID; }
        return OBIA_OK;
    }
    int count(const char *name, int64_t n, int64_t least) const {
        if (n < least) { set_error("%s: %s: %s must be at least %lld, got %lld", module, what, name, (long long)least, (long long)n); return OBIA_E_INVALID; }
        if (n > (int64_t)INT32_MAX) { set_error("%s: %s: %s must be below 2^31, got %lld", module, what, name, (long long)n); return OBIA_E_UNSUPPORTED; }
        return OBIA_OK;
    }
};

}  // namespace obia
