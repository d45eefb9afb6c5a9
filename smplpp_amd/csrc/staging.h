// Host/device argument staging for the non-hot entry points (stage-level ops, mesh queries, setters/getters, the host form of
// smplpp_fk and of the backward passes).  A host-space argument goes through `buf` when one is given (a persistent per-handle
// buffer, grown as needed), else through a temporary freed with the In / Out.
#pragma once
#include "common.h"

namespace smplpp_hip
{
// An input that must be readable on the device: either the caller's device pointer or an upload.
template<class T>
struct In
{
  const T * d = nullptr;
  DevPtr<T> tmp;
  hipError_t init(const T * p, size_t count, int space, hipStream_t st, DevBuf * buf = nullptr)
  {
    if(!p || count == 0) return hipSuccess;
    if(space == SMPLPP_DEVICE)
    {
      d = p;
      return hipSuccess;
    }
    hipError_t e = buf ? buf->reserve(sizeof(T) * count) : dev_alloc(tmp, count);
    if(e != hipSuccess) return e;
    T * dst = buf ? buf->as<T>() : tmp.get();
    d = dst;
    return hipMemcpyAsync(dst, p, sizeof(T) * count, hipMemcpyHostToDevice, st);
  }
};

// An output: the caller's device pointer, or a device copy that finish() copies back.
template<class T>
struct Out
{
  T * d = nullptr;
  DevPtr<T> tmp;
  T * host = nullptr;
  size_t count = 0;
  hipError_t init(T * p, size_t cnt, int space, DevBuf * buf = nullptr)
  {
    if(!p || cnt == 0) return hipSuccess;
    count = cnt;
    if(space == SMPLPP_DEVICE)
    {
      d = p;
      return hipSuccess;
    }
    host = p;
    hipError_t e = buf ? buf->reserve(sizeof(T) * cnt) : dev_alloc(tmp, cnt);
    if(e == hipSuccess) d = buf ? buf->as<T>() : tmp.get();
    return e;
  }
  // the caller's host values into the device copy (an output the call adds into)
  hipError_t load(hipStream_t st)
  {
    if(!host) return hipSuccess;
    return hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, st);
  }
  hipError_t finish(hipStream_t st)
  {
    if(!host) return hipSuccess;
    return hipMemcpyAsync(host, d, sizeof(T) * count, hipMemcpyDeviceToHost, st);
  }
};

inline int check_space(int space, const char * fn)
{
  if(space != SMPLPP_HOST && space != SMPLPP_DEVICE) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad memory space");
  return SMPLPP_OK;
}
} // namespace smplpp_hip
