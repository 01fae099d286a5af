// Error plumbing and host/device staging shared by the C-ABI translation units (engine.cpp, vf.cpp,
// standalone.cpp): every exported entry runs its body under guarded(), which maps the exception
// type to the TRPO_ERR_* code and keeps the message for trpo_last_error().
#pragma once
#include "../../include/trpo_engine.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace trpo_abi {

inline thread_local std::string g_last_error;

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct ArgError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct RcclError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHECK(x)                                                                       \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      throw ::trpo_abi::HipError(std::string(#x) + " failed: " + hipGetErrorString(e_));  \
  } while (0)
#define NCCLCHECK(x)                                                                      \
  do {                                                                                    \
    ncclResult_t r_ = (x);                                                                \
    if (r_ != ncclSuccess)                                                                \
      throw ::trpo_abi::RcclError(std::string(#x) + " failed: " + ncclGetErrorString(r_)); \
  } while (0)
#define REQUIRE(c, msg)                          \
  do {                                           \
    if (!(c)) throw ::trpo_abi::ArgError(msg);   \
  } while (0)

template <class F>
int guarded(F&& f) {
  try {
    f();
    return TRPO_OK;
  } catch (const ArgError& e) {
    g_last_error = e.what();
    return TRPO_ERR_ARG;
  } catch (const RcclError& e) {
    g_last_error = e.what();
    return TRPO_ERR_RCCL;
  } catch (const HipError& e) {
    g_last_error = e.what();
    return TRPO_ERR_HIP;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return TRPO_ERR_STATE;
  }
}

inline int pad4(int x) { return (x + 3) & ~3; }

inline void check_launch() { HIPCHECK(hipGetLastError()); }

// Split-K geometry of the weight-gradient slabs (SlabDst) for n rows over at most `splits` slabs: rows per split,
// a multiple of the largest wgrad k-tile (32 rows) and >= 64, and the splits that then hold rows
struct SplitGeom {
  int rows_per_split, active;
};
inline SplitGeom split_geometry(int64_t n, int splits) {
  const int64_t rps = std::max<int64_t>(64, ((n + splits - 1) / splits + 31) / 32 * 32);
  return SplitGeom{(int)rps, (int)std::max<int64_t>(1, (n + rps - 1) / rps)};
}

// caller pointer (host or device, TRPO_MEM_*) -> device buffer on `s`; host copies are
// synchronous so the caller may free its buffer on return
inline void copy_in(void* dst, const void* src, size_t bytes, int mem, hipStream_t s) {
  if (bytes == 0) return;
  HIPCHECK(hipMemcpyAsync(dst, src, bytes, mem == TRPO_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          s));
  if (mem != TRPO_MEM_DEVICE) HIPCHECK(hipStreamSynchronize(s));
}
inline void copy_out(void* dst, const void* src, size_t bytes, int mem, hipStream_t s) {
  if (bytes == 0) return;
  HIPCHECK(hipMemcpyAsync(dst, src, bytes, mem == TRPO_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          s));
  HIPCHECK(hipStreamSynchronize(s));
}

// Device staging of one C-ABI call's caller arrays (mem = TRPO_MEM_*) on stream `s`: a device array is used in
// place, a host array gets a device temporary (inputs copied in at once, outputs copied back by fetch()); NULL
// stays NULL.  The destructor frees every temporary, so nothing leaks when a launch or a copy throws.
class Staging {
 public:
  Staging(int mem, hipStream_t s) : host_(mem != TRPO_MEM_DEVICE), s_(s) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    for (void* p : bufs_) (void)hipFree(p);
  }
  template <class T>
  T* tmp(size_t count) {   // a device temporary (uninitialised)
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    bufs_.push_back(p);
    return static_cast<T*>(p);
  }
  template <class T>
  const T* in(const T* src, size_t count) {
    if (!src || !host_) return src;
    T* d = tmp<T>(count);
    copy_in(d, src, count * sizeof(T), TRPO_MEM_HOST, s_);
    return d;
  }
  template <class T>
  T* out(T* dst, size_t count) {
    if (!dst || !host_) return dst;
    T* d = tmp<T>(count);
    outs_.push_back(Out{dst, d, count * sizeof(T)});
    return d;
  }
  template <class T>
  T* inout(T* p, size_t count) {   // read and written in place
    T* d = out(p, count);
    if (d != p) copy_in(d, p, count * sizeof(T), TRPO_MEM_HOST, s_);
    return d;
  }
  // the host outputs, once the work is enqueued on the stream; each copy waits for the stream
  void fetch() {
    for (const Out& o : outs_) copy_out(o.host, o.dev, o.bytes, TRPO_MEM_HOST, s_);
  }

 private:
  struct Out {
    void* host;
    const void* dev;
    size_t bytes;
  };
  bool host_;
  hipStream_t s_;
  std::vector<void*> bufs_;
  std::vector<Out> outs_;
};

}  // namespace trpo_abi
