// at2v_device_scope.h — the caller's current HIP device, saved for a scope (the context code and the queue backend).
//
// Every entry point that sets a device restores the caller's on every return path: with launches from the producer's
// thread (at2v_queue_submit in latency mode) a user thread must not find its HIP device switched.
#pragma once
#include <hip/hip_runtime.h>

namespace at2v {

struct DeviceScope {
  int prev = -1;
  hipError_t err = hipSuccess;
  // save only: a scope that sets a device per shard itself (the multi-device entry points)
  DeviceScope() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  // save, then make `device` the current one (err: what setting it returned)
  explicit DeviceScope(int device) : DeviceScope() { err = prev == device ? hipSuccess : hipSetDevice(device); }
  ~DeviceScope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace at2v
