// One owning buffer type for every device and pinned allocation of a context.  No HIP here: the memory comes from a policy
// with two static functions, `void *alloc(size_t bytes)` (nullptr: failed) and `void free(void *)` -- fs3d_common.h has the
// device and the pinned one, tests/dev_buffer_test.cpp one over malloc that counts and can be told to fail.
#pragma once
#include <stddef.h>
#include <initializer_list>

// A pointer and the bytes it holds: empty (null, 0) or allocated, never a stale pointer or a stale capacity.  Move-only.
// `count`, where given, gains 1 per allocation and 1 per free of a non-null buffer (fs3d_geometry_info entry 13).
template <class Mem>
class RawBuf {
    void *p_ = nullptr;
    size_t bytes_ = 0;
public:
    RawBuf() = default;
    RawBuf(RawBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    RawBuf &operator=(RawBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~RawBuf() { reset(); }
    void *raw() const { return p_; }
    size_t bytes() const { return bytes_; }
    bool holds(size_t bytes) const { return p_ && bytes_ >= bytes; }
    void reset(long long *count = nullptr)
    {
        if (p_) { Mem::free(p_); if (count) ++*count; }
        p_ = nullptr; bytes_ = 0;
    }
    // exactly `bytes`, always a new allocation; false: failed, and the buffer is empty
    bool replace(size_t bytes, long long *count = nullptr)
    {
        reset(count);
        if (!(p_ = Mem::alloc(bytes))) return false;
        bytes_ = bytes;
        if (count) ++*count;
        return true;
    }
    // at least `bytes`, grow-only; the old contents are not kept.  *fresh is set where it allocated (the caller may have to clear)
    bool reserve(size_t bytes, long long *count = nullptr, bool *fresh = nullptr)
    {
        if (holds(bytes)) return true;
        if (fresh) *fresh = true;
        return replace(bytes, count);
    }
};

// ... of elements T: reads as a T * wherever one is expected (kernel arguments, arithmetic, tests for null), and under a cast
// as a pointer to any other type
template <class Mem, class T = void>
struct OwnedBuf : RawBuf<Mem> {
    operator T *() const { return static_cast<T *>(this->raw()); }
    template <class U> explicit operator U *() const { return static_cast<U *>(this->raw()); }
};

// all or nothing: every buffer of the set holds its bytes, or -- one allocation failed -- all of them are empty
template <class Mem> struct BufWant { RawBuf<Mem> *buf; size_t bytes; };
template <class Mem>
bool reserve_all(std::initializer_list<BufWant<Mem>> set, long long *count = nullptr, bool *fresh = nullptr)
{
    for (const BufWant<Mem> &w : set)
        if (!w.buf->reserve(w.bytes, count, fresh)) {
            for (const BufWant<Mem> &v : set) v.buf->reset(count);
            return false;
        }
    return true;
}
