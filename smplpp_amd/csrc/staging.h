// Host/device argument staging: one Frame per entry point that takes a memory space (stage-level ops, mesh queries, the scan and
// image terms, setters/getters, the host form of smplpp_fk and of the backward passes).  A handle owns an Arena of device buffers;
// the k-th argument a host-space call STAGES (uploads, or receives on the device to copy back) goes through slot k, whatever its
// type and whichever entry point is running.  "One caller thread per handle" and the synchronisation that ends every host-space
// call make a slot free again when the call returns.  An argument that is not staged — a null pointer, a zero count, a device
// pointer — takes no slot.  A frame without an arena (the handle-less entry points) stages through an arena of its own, freed
// with the frame.  In device space a frame costs the hipSetDevice its entry point always made: no allocation, no other HIP call.
// The one exception is smplpp_sweep_grid, whose six floats of bounds scratch come from slot 0 of the model's arena in either space.
// A getter or setter of state the handle keeps on the device (the IK solver's configuration, tasks, step, status, mesh) stages
// nothing: fetch() / store() copy between the handle's array and the caller's, in the frame's space, on the frame's stream.
#pragma once
#include "common.h"
#include "trace.h"

namespace smplpp_hip
{
inline int check_space(int space, const char * fn)
{
  if(space != SMPLPP_HOST && space != SMPLPP_DEVICE) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad memory space");
  return SMPLPP_OK;
}

// host-side check of host-space ids: every one in [lo, bound)
inline int ids_in(const char * fn, const char * what, const int64_t * ids, int64_t count, int64_t lo, int64_t bound)
{
  for(int64_t i = 0; i < count; i++)
    if(ids[i] < lo || ids[i] >= bound) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + what + " out of range");
  return SMPLPP_OK;
}

// The call frame of one entry point: selects the device, opens the trace range (name may be null), hands out device pointers for
// the arguments, copies between the handle's own device arrays and the caller's (fetch / store), and in run() / finish() copies
// the staged host-space outputs back in the order they were declared and synchronises.
// The first HIP error sticks: every later request is a no-op giving null, and run() reports it without calling its body, under
// the name and the place of the entry point that built the frame.
class Frame
{
 public:
  const hipStream_t st;

  Frame(int device, Arena * arena, int space, void * stream, const char * trace, const char * fn = __builtin_FUNCTION(),
        const char * file = __builtin_FILE(), int line = __builtin_LINE())
      : st(static_cast<hipStream_t>(stream)), e_(hipSetDevice(device)), tr_(e_ == hipSuccess ? trace : nullptr),
        arena_(arena ? arena : &own_), space_(space), fn_(fn), file_(file), line_(line)
  {
  }
  Frame(const Frame &) = delete;
  Frame & operator=(const Frame &) = delete;

  // an input readable on the device: the caller's device pointer, or an upload
  template<class T>
  const T * in(const T * p, size_t count)
  {
    if(space_ == SMPLPP_DEVICE) return count ? p : nullptr;
    return upload(p, count);
  }
  // a host array in either space (a table the entry point built itself)
  template<class T>
  const T * upload(const T * p, size_t count)
  {
    T * d = p ? scratch<T>(count) : nullptr;
    if(d) note(hipMemcpyAsync(d, p, sizeof(T) * count, hipMemcpyHostToDevice, st), "hipMemcpyAsync (stage an input)");
    return e_ == hipSuccess ? d : nullptr;
  }
  // an output: the caller's device pointer, or a device copy that finish() copies back; `load` first uploads the caller's values
  // (an output the call adds into)
  template<class T>
  T * out(T * p, size_t count, bool load = false)
  {
    if(space_ == SMPLPP_DEVICE) return count ? p : nullptr;
    T * d = p ? scratch<T>(count) : nullptr;
    if(!d) return nullptr;
    back_[nback_++] = {p, d, sizeof(T) * count};
    if(load) note(hipMemcpyAsync(d, p, sizeof(T) * count, hipMemcpyHostToDevice, st), "hipMemcpyAsync (load an output)");
    return e_ == hipSuccess ? d : nullptr;
  }
  // device memory of the call's own, in either space
  template<class T>
  T * scratch(size_t count)
  {
    if(e_ != hipSuccess || count == 0) return nullptr;
    if(next_ == ARENA_SLOTS)
    {
      note(hipErrorInvalidValue, "Frame: more staged arguments than ARENA_SLOTS");
      return nullptr;
    }
    DevBuf & b = arena_->slot[next_];
    if(!note(b.reserve(sizeof(T) * count), "hipMalloc (staging slot)")) return nullptr;
    next_++;
    return b.as<T>();
  }
  // a device array the handle owns -> the caller's array in the frame's space, enqueued here (no slot; finish() synchronises a
  // host-space call); a null caller pointer or a zero count: nothing
  template<class T>
  void fetch(T * caller_dst, const T * dev_src, size_t count)
  {
    if(caller_dst && count && e_ == hipSuccess)
      note(hipMemcpyAsync(caller_dst, dev_src, sizeof(T) * count, space_ == SMPLPP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st),
           "hipMemcpyAsync (fetch from the handle)");
  }
  // the other way: the caller's array -> a device array the handle owns
  template<class T>
  void store(T * dev_dst, const T * caller_src, size_t count)
  {
    if(caller_src && count && e_ == hipSuccess)
      note(hipMemcpyAsync(dev_dst, caller_src, sizeof(T) * count, space_ == SMPLPP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st),
           "hipMemcpyAsync (store into the handle)");
  }
  // false once a HIP call of the frame has failed (ask before creating state on the device the frame selected)
  bool ok() const { return e_ == hipSuccess; }
  // wait for the stream in mid-call (before a host read of what the call has computed so far)
  bool sync() { return e_ == hipSuccess && note(hipStreamSynchronize(st), "hipStreamSynchronize"); }

  // body() on the staged pointers (an int status: nonzero is returned as it is), then finish()
  template<class Body>
  int run(Body && body)
  {
    if(e_ == hipSuccess)
      if(int rc = body()) return rc;
    return finish();
  }
  // the copies back, then the synchronisation that ends a host-space call, or one that used the frame's own arena in device space
  int finish()
  {
    for(int i = 0; i < nback_ && e_ == hipSuccess; i++)
      note(hipMemcpyAsync(back_[i].host, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (copy an output back)");
    nback_ = 0;
    if(space_ == SMPLPP_HOST || (next_ > 0 && arena_ == &own_)) sync();
    return e_ == hipSuccess ? SMPLPP_OK : hip_fail(e_, (std::string(fn_) + ": " + what_).c_str(), file_, line_);
  }

 private:
  bool note(hipError_t e, const char * what)
  {
    if(e != hipSuccess && e_ == hipSuccess) e_ = e, what_ = what;
    return e == hipSuccess;
  }
  struct Back
  {
    void * host;
    const void * dev;
    size_t bytes;
  };
  hipError_t e_;                     // (in front of tr_: the device is selected first, and no range opens when that fails)
  const char * what_ = "hipSetDevice"; // what the first failure was doing
  TraceRange tr_;
  Arena own_; // stays empty when the handle lends its arena
  Arena * arena_;
  Back back_[ARENA_SLOTS];
  int space_, next_ = 0, nback_ = 0;
  const char *fn_, *file_;
  int line_;
};
} // namespace smplpp_hip
