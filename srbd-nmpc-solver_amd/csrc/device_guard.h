// device_guard.h -- makes a device current for a scope and restores the caller's on exit.
#pragma once

#include <hip/hip_runtime.h>

namespace srbd {

class __attribute__((visibility("hidden"))) DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    (void)hipGetDevice(&prev_);
    status_ = hipSetDevice(device);
  }
  ~DeviceGuard() { (void)hipSetDevice(prev_); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  hipError_t status() const { return status_; }  // of the switch

 private:
  int prev_ = 0;
  hipError_t status_ = hipSuccess;
};

}  // namespace srbd
