// One device allocation carved into typed arrays.  Every array is named ONCE -- add(&ptr, count) -- and both the total
// byte count and every pointer come from that list: bytes() after the last add(), bind(base) once the memory is there.
// Each array starts at a multiple of alignof(T); a zero count adds no bytes and gets a pointer nobody dereferences.
// The layout part is plain C++ (no HIP call, no heap); the owning block and the typed copies need hipcc.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace smooth_feedback_amd::detail {

class DeviceArena {
public:
  static constexpr int kCapacity = 24;  // the largest call site declares 14 arrays

  /// declare `count` elements of T; *slot is set by bind().  Past kCapacity: nothing is recorded, ok() turns false.
  template<class T>
  int add(T ** slot, std::size_t count)
  {
    *slot = nullptr;
    if (n_ == kCapacity) return overflow_ = true, -1;
    const std::size_t at = (bytes_ + alignof(T) - 1) / alignof(T) * alignof(T);
    e_[n_] = {slot, at, count * sizeof(T)};
    if (count) bytes_ = at + count * sizeof(T);
    return n_++;
  }
  bool ok() const { return !overflow_; }
  int size() const { return n_; }
  std::size_t bytes() const { return bytes_; }
  std::size_t bytes(int i) const { return e_[i].bytes; }
  void * at(int i) const { return base_ + e_[i].offset; }
  /// hand every declared pointer its address in [base, base + bytes()); base: aligned for the widest T (hipMalloc's is)
  bool bind(void * base)
  {
    if (overflow_) return false;
    base_ = static_cast<char *>(base);
    for (int i = 0; i < n_; ++i) {
      void * p = base_ + e_[i].offset;
      std::memcpy(e_[i].slot, &p, sizeof p);  // (a T* variable, whatever T)
    }
    return true;
  }

private:
  struct Entry { void * slot; std::size_t offset, bytes; };
  Entry e_[kCapacity];
  int n_             = 0;
  std::size_t bytes_ = 0;
  char * base_       = nullptr;
  bool overflow_     = false;
};

}  // namespace smooth_feedback_amd::detail

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <utility>

namespace smooth_feedback_amd::detail {

/// "<who>: <what>: <HIP's text>" as std::runtime_error
inline void hip_check(hipError_t e, const char * who, const char * what)
{
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
}

/// owns one hipMalloc; error() tells how it went (no exception: the C entry points report by status)
class DeviceBlock {
public:
  DeviceBlock() = default;
  explicit DeviceBlock(std::size_t bytes) { e_ = hipMalloc(&p_, bytes ? bytes : 1); }
  /// the block of an arena, bound to it; throws hip_check's error under `who`
  DeviceBlock(DeviceArena & a, const char * who) : DeviceBlock(a.bytes())
  {
    if (!a.ok()) throw std::length_error(std::string(who) + ": more arrays than DeviceArena holds");
    hip_check(e_, who, "hipMalloc");
    a.bind(p_);
  }
  DeviceBlock(DeviceBlock && o) noexcept { *this = std::move(o); }
  DeviceBlock & operator=(DeviceBlock && o) noexcept { return std::swap(p_, o.p_), std::swap(e_, o.e_), *this; }  // (o frees ours)
  ~DeviceBlock() { if (p_) (void)hipFree(p_); }
  void * get() const { return p_; }
  hipError_t error() const { return e_; }

private:
  void * p_     = nullptr;
  hipError_t e_ = hipSuccess;
};

template<class T>
inline hipError_t upload(T * dst, const T * src, std::size_t count) { return hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice); }
template<class T>
inline hipError_t download(T * dst, const T * src, std::size_t count) { return hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost); }

/// one lane per item, 64 to a block
inline dim3 lane_grid(int64_t B) { return dim3((unsigned)((B + 63) / 64)); }

}  // namespace smooth_feedback_amd::detail
#endif
