// ea_launch.h -- the per-device launch state of libea_hip.so (host side; ea_common.h includes it).
//
// hipFuncSetAttribute acts on the CURRENT device's copy of a kernel, and the CU count and a kernel's occupancy are device
// properties: a process that drives several GPUs must keep all three per device.  Forward and backward launches
// come from different threads under autograd, so the three tables share one mutex.  These three functions are the only
// callers of hipGetDeviceProperties, hipFuncSetAttribute and hipOccupancyMaxActiveBlocksPerMultiprocessor in the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <tuple>

namespace ea {

constexpr int EA_MAX_DEV = 64;
constexpr int EA_LDS_DEFAULT_LIMIT = 64 * 1024;      // dynamic LDS a launch may ask for without a hipFuncSetAttribute call

struct LaunchState {
  std::mutex mu;
  int cus[EA_MAX_DEV] = {};
  std::map<std::pair<int, const void*>, int> lds_limit;                  // (device, kernel) -> bytes last granted
  std::map<std::tuple<int, const void*, int, size_t>, int> occupancy;    // (device, kernel, threads, dynamic LDS) -> workgroups per CU
};
inline LaunchState& ea_launch_state() {
  static LaunchState s;
  return s;
}
inline int ea_cur_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EA_MAX_DEV) dev = 0;
  return dev;
}

// CUs of the current device (256 = MI355X when no device is visible, e.g. build checks)
inline int ea_device_cus() {
  LaunchState& s = ea_launch_state();
  const int dev = ea_cur_device();
  std::lock_guard<std::mutex> lock(s.mu);
  if (!s.cus[dev]) {
    hipDeviceProp_t prop;
    int v = 0;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) v = prop.multiProcessorCount;
    s.cus[dev] = v > 0 ? v : 256;
  }
  return s.cus[dev];
}

// Make sure the current device's copy of `kernel` may be launched with `bytes` of dynamic LDS.  The limit is a high-water
// mark per (device, kernel) that starts at the 64 KB every kernel has: the driver is called only when `bytes` exceeds what
// this kernel was last given here, so a kernel whose image depends on a run-time size (pf32_lds(which, M), kz_lds_floats(map, M))
// is raised again when a larger size arrives and never lowered.  Keyed by the kernel's host address, not by the call site:
// one site may pick its kernel at run time.  -> hipError_t as int (the mark moves only on success).
inline int ea_lds_limit(const void* kernel, size_t bytes) {
  LaunchState& s = ea_launch_state();
  const int dev = ea_cur_device();
  std::lock_guard<std::mutex> lock(s.mu);
  int& mark = s.lds_limit.emplace(std::make_pair(dev, kernel), EA_LDS_DEFAULT_LIMIT).first->second;
  if (bytes <= (size_t)mark) return (int)hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) mark = (int)bytes;
  return (int)e;
}
template <typename K> int ea_lds_limit(K* kernel, size_t bytes) { return ea_lds_limit(reinterpret_cast<const void*>(kernel), bytes); }

// Resident workgroups per CU of `kernel` launched with `threads` threads and `bytes` of dynamic LDS on the current device
// (2 when the runtime cannot say).
inline int ea_occupancy(const void* kernel, int threads, size_t bytes) {
  LaunchState& s = ea_launch_state();
  const int dev = ea_cur_device();
  std::lock_guard<std::mutex> lock(s.mu);
  int& occ = s.occupancy[std::make_tuple(dev, kernel, threads, bytes)];
  if (!occ) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, bytes) != hipSuccess || n <= 0) n = 2;
    occ = n;
  }
  return occ;
}
template <typename K> int ea_occupancy(K* kernel, int threads, size_t bytes) {
  return ea_occupancy(reinterpret_cast<const void*>(kernel), threads, bytes);
}

// integer dev knob from the environment (callers keep the value in a function-local static: read once)
inline int ea_env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return s ? atoi(s) : dflt;
}

}  // namespace ea
