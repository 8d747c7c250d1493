// rover_operands.h — the argument checks every learning entry point of the C layer shares: an entry point lists the arrays it was handed as
// a small table of operands, and one function applies the operand rules of include/rover_step.h to it and writes the refusal.
// Host only, plain C++: no HIP, no rover_ctx, no heap (rover_gru_cell runs thousands of times per BPTT pass).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace rover {

constexpr int64_t kMaxRowStride = (int64_t)1 << 40;        // elements
constexpr uint64_t kMaxExtentBytes = (uint64_t)1 << 62;    // rows x stride x size of one operand; the one place that keeps the sums below from wrapping

struct Span { uintptr_t lo, hi; };      // the bytes [lo, hi) of an array

inline bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

// The bytes a [rows, cols] array of `size`-byte elements at a row stride (in elements, 0: one row serves every row) covers; nothing when it
// has no element.  False, and an empty span, when rows x max(stride, cols) x size passes kMaxExtentBytes or the span would pass the end of
// the address space: with the bound, no product or sum here can wrap.
inline bool span_of(const void* p, int64_t stride, int64_t rows, int64_t cols, size_t size, Span* out) {
    const uintptr_t lo = (uintptr_t)p;
    *out = Span{lo, lo};
    if (rows <= 0 || cols <= 0) return true;
    uint64_t padded;                    // rows x max(stride, cols) x size, without a division: this runs for every operand of every call
    if (__builtin_mul_overflow((uint64_t)rows, (uint64_t)(stride > cols ? stride : cols), &padded) || __builtin_mul_overflow(padded, (uint64_t)size, &padded) ||
        padded > kMaxExtentBytes)
        return false;
    const uint64_t bytes = ((uint64_t)(rows - 1) * (uint64_t)(stride > 0 ? stride : 0) + (uint64_t)cols) * size;
    if (lo + bytes < lo) return false;
    out->hi = lo + bytes;
    return true;
}

enum OperandRole : uint8_t {
    OP_READ,        // may overlap other read operands
    OP_WRITTEN,     // overlaps nothing, but for a declared same-array pair
    OP_STATE        // read and written, or a record that has to stand clear of every array like one: checked as OP_WRITTEN
};
enum : uint32_t {
    OP_OPTIONAL = 1u,       // a NULL pointer takes the operand out of every check
    OP_STRIDE0 = 2u,        // a row stride of 0 is accepted as well
    OP_BYTES = 4u           // cols is the extent in bytes (one row; stride and size are not looked at)
};

struct Operand {
    const char* name;       // as in rover_step.h
    const void* p;
    int64_t stride;         // row stride in elements
    int64_t rows, cols;
    uint32_t size;          // of an element, in bytes
    OperandRole role;
    uint32_t flags;
    uint32_t align;         // required alignment of p in bytes, a power of two; 0: none
};

// The table of one call, on the stack; an operand the call does not look at is simply not added.  refused() applies the six operand rules
// of rover_step.h, each over the whole table before the next.  An overlap is reported as "<entry>: <later> overlaps <earlier>", by the
// operands' order in the table.
class Operands {
  public:
    static constexpr int kCapacity = 16;
    explicit Operands(const char* entry) : entry_(entry) {}
    const char* entry() const { return entry_; }

    Operands& add(OperandRole role, const char* name, const void* p, int64_t stride, int64_t rows, int64_t cols, uint32_t size, uint32_t flags = 0,
                  uint32_t align = 0) {
        if (n_ == kCapacity) { full_ = true; return *this; }
        Operand& o = op_[n_++];
        o.name = name; o.p = p; o.stride = stride; o.rows = rows; o.cols = cols; o.size = size; o.role = role; o.flags = flags; o.align = align;
        return *this;
    }
    template <typename... A> Operands& read(A... a) { return add(OP_READ, a...); }
    template <typename... A> Operands& written(A... a) { return add(OP_WRITTEN, a...); }
    template <typename... A> Operands& state(A... a) { return add(OP_STATE, a...); }
    // `a` and `b` (names of the table) may be the same array
    Operands& same_array(const char* a, const char* b) { alias_a_ = a; alias_b_ = b; return *this; }

    // True, with the refusal in msg, when the table breaks a rule
    bool refused(char* msg, size_t cap) {
        if (full_) return say(msg, cap, "more than %d operands", kCapacity);
        bool live[kCapacity];           // given: takes part in rules 2 and 3
        bool spans[kCapacity];          // given and with elements: takes part in rules 4 to 6
        for (int i = 0; i < n_; ++i) {
            const Operand& o = op_[i];
            const bool empty = o.rows <= 0 || o.cols <= 0;
            live[i] = o.p || !(o.flags & OP_OPTIONAL);
            spans[i] = o.p && !empty;
            if (!o.p && live[i] && !empty) return say_null(msg, cap, o);
        }
        for (int i = 0; i < n_; ++i) {
            const Operand& o = op_[i];
            if (!live[i] || (o.flags & OP_BYTES)) continue;
            const bool zero_ok = (o.flags & OP_STRIDE0) && o.stride == 0;
            if (!zero_ok && (o.stride < o.cols || o.stride > kMaxRowStride))
                return say(msg, cap, "the row stride of %s (%lld) is %s its row (%lld) or above 2^40", o.name, (long long)o.stride,
                           (o.flags & OP_STRIDE0) ? "neither 0 nor at least" : "shorter than", (long long)o.cols);
        }
        for (int i = 0; i < n_; ++i)
            if (live[i] && op_[i].align && ((uintptr_t)op_[i].p & (op_[i].align - 1))) return say(msg, cap, "%s is not %u-byte aligned", op_[i].name, op_[i].align);
        Span* s = span_;
        for (int i = 0; i < n_; ++i) {
            const Operand& o = op_[i];
            const bool bytes = o.flags & OP_BYTES;
            if (spans[i] && !span_of(o.p, bytes ? o.cols : o.stride, bytes ? 1 : o.rows, o.cols, bytes ? 1 : o.size, &s[i]))
                return say(msg, cap, "%s: extent too large (rows x stride x size above 2^62 bytes)", o.name);
        }
        int wi = -1, wj = -1;           // the first pair of written operands that overlaps: reported when no written / read pair does
        for (int i = 1; i < n_; ++i) {
            if (!spans[i]) continue;
            for (int j = 0; j < i; ++j) {
                const int n_written = (op_[i].role != OP_READ) + (op_[j].role != OP_READ);
                if (!spans[j] || n_written == 0 || !overlap(s[i], s[j])) continue;
                if (may_alias(op_[i], op_[j]) && op_[i].p == op_[j].p && op_[i].stride == op_[j].stride) continue;
                if (n_written == 1) return say_overlap(msg, cap, i, j);
                if (wi < 0) { wi = i; wj = j; }
            }
        }
        return wi >= 0 && say_overlap(msg, cap, wi, wj);
    }

    Span span(int i) const { return span_[i]; }        // of operand i, after a refused() that returned false

  private:
    template <typename... A>
    bool say(char* msg, size_t cap, const char* fmt, A... a) const {
        const int k = snprintf(msg, cap, "%s: ", entry_);
        if (k >= 0 && (size_t)k < cap) snprintf(msg + k, cap - (size_t)k, fmt, a...);
        return true;
    }
    // "<entry>: x must be given (null pointer; the call needs x, w and y)"
    bool say_null(char* msg, size_t cap, const Operand& o) const {
        char need[256] = "";
        size_t at = 0;
        int left = 0;
        for (int i = 0; i < n_; ++i) left += !(op_[i].flags & OP_OPTIONAL);
        for (int i = 0; i < n_ && at < sizeof need; ++i) {
            if (op_[i].flags & OP_OPTIONAL) continue;
            --left;
            const int k = snprintf(need + at, sizeof need - at, "%s%s", op_[i].name, left > 1 ? ", " : left == 1 ? " and " : "");
            if (k < 0) break;
            at += (size_t)k;
        }
        return say(msg, cap, "%s must be given (null pointer; the call needs %s)", o.name, need);
    }
    bool say_overlap(char* msg, size_t cap, int i, int j) const {
        return say(msg, cap, "%s overlaps %s%s", op_[i].name, op_[j].name,
                   may_alias(op_[i], op_[j]) ? " without being the same array (same pointer and stride)" : "");
    }
    bool may_alias(const Operand& a, const Operand& b) const {
        if (!alias_a_) return false;
        return (!strcmp(a.name, alias_a_) && !strcmp(b.name, alias_b_)) || (!strcmp(a.name, alias_b_) && !strcmp(b.name, alias_a_));
    }

    const char* entry_;
    Operand op_[kCapacity];
    Span span_[kCapacity];
    int n_ = 0;
    bool full_ = false;
    const char* alias_a_ = nullptr;
    const char* alias_b_ = nullptr;
};

}  // namespace rover
