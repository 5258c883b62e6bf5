// The one owner of device memory: the Engine's key, table and scratch members and the staging scope of an entry
// point (model.cpp) hold their allocations in a DevBuf.  Host code only; compiles under hipcc and the host compiler.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <type_traits>

namespace tae {

struct HipError {
    std::string msg;
};

void hip_check(hipError_t e, const char *what);

// A pointer and a capacity in elements.  Move-only; converts to T * so that launches and `d_x_ + offset` read as
// they do for a raw pointer (get() where an argument's type is deduced).  Memory set by borrow() is the caller's.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_), owned_(o.owned_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p_, o.p_), std::swap(cap_, o.cap_), std::swap(owned_, o.owned_);
        return *this;
    }
    ~DevBuf() {
        if (p_ && owned_) (void)hipFree(p_);
    }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }

    // frees what is held and allocates count elements (at least 16 bytes); contents are not kept
    T *alloc(size_t count) {
        T *old = owned_ ? p_ : nullptr;
        p_ = nullptr, cap_ = 0, owned_ = true;  // a failure below leaves nothing for the destructor
        if (old) hip_check(hipFree(old), "hipFree");
        hip_check(hipMalloc((void **)&p_, std::max<size_t>(count * sizeof(T), 16)), "hipMalloc");
        cap_ = count;
        return p_;
    }
    // grow-only: reallocates when count exceeds the capacity, and only then
    T *grow(size_t count) { return count > cap_ ? alloc(count) : p_; }
    // grow, then the asynchronous copy of count host elements; `host` must live until the stream has read it
    T *upload(const T *host, size_t count, hipStream_t stream) {
        grow(count);
        if (count) hip_check(hipMemcpyAsync(p_, host, count * sizeof(T), hipMemcpyHostToDevice, stream), "upload");
        return p_;
    }
    // memory the caller owns and keeps valid: never freed here
    void borrow(T *p) {
        if (p_ && owned_) hip_check(hipFree(p_), "hipFree");
        p_ = p, cap_ = 0, owned_ = false;
    }

  private:
    T *p_ = nullptr;
    size_t cap_ = 0;
    bool owned_ = true;
};

static_assert(!std::is_copy_constructible<DevBuf<char>>::value && !std::is_copy_assignable<DevBuf<char>>::value,
              "a DevBuf has one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf<char>>::value &&
                  std::is_nothrow_move_assignable<DevBuf<char>>::value,
              "a DevBuf moves without allocating");

}  // namespace tae
