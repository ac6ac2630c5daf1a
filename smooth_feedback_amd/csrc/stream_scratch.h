// Working memory of one launch sequence on a stream, owned for exactly that long.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace sfb {

// The caller's workspace when there is one (or nothing to hold): owns nothing.  Otherwise a stream-ordered allocation (no
// device synchronisation in the steady state), hipMalloc where the device has no memory pool.  Freed on every exit path,
// behind the launches already on the stream: hipFreeAsync, or (fallback) hipStreamSynchronize + hipFree.
// One rule for every user -- the first error wins: error() of the allocation, then the launches, then release().
class StreamScratch {
public:
  StreamScratch(void *callers_workspace, size_t bytes, hipStream_t stream) : p_(callers_workspace), stream_(stream)
  {
    if (callers_workspace || !bytes) return;
    e_ = hipMallocAsync(&p_, bytes, stream);
    if (e_ != hipSuccess) {
      (void)hipGetLastError();
      async_ = false;
      e_     = hipMalloc(&p_, bytes);
    }
    owned_ = e_ == hipSuccess;
    if (!owned_) p_ = nullptr;
  }
  StreamScratch(const StreamScratch &)            = delete;
  StreamScratch &operator=(const StreamScratch &) = delete;
  ~StreamScratch() { (void)release(); }
  void *get() const { return p_; }
  hipError_t error() const { return e_; }
  // free now (what the destructor does otherwise); the error of the free
  hipError_t release()
  {
    if (!owned_) return hipSuccess;
    owned_ = false;
    if (async_) return hipFreeAsync(p_, stream_);
    (void)hipStreamSynchronize(stream_);
    return hipFree(p_);
  }

private:
  void *p_;
  hipStream_t stream_;
  hipError_t e_ = hipSuccess;
  bool owned_ = false, async_ = true;
};

}  // namespace sfb
