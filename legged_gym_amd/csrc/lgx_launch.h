// Host-side launch helpers shared by the GEMM / MLP / PPO translation units.  lgx_xcd_grid is
// plain C++ (tests/test_split_bf16_host.py compiles it with the host compiler).
#pragma once
#include <stdint.h>

#include <algorithm>

// Grid of a persistent kernel over `tiles` tiles: at most wgs_per_cu workgroups per CU, and a
// multiple of 8 - workgroup b runs on XCD b % 8 and walks that XCD's contiguous eighth of the tile
// range with stride grid / 8 (neighbouring tiles share operand rows in one XCD's L2).
inline int64_t lgx_xcd_grid(int64_t tiles, int cus, int wgs_per_cu) {
  return 8 * std::min<int64_t>((tiles + 7) / 8, std::max(1, wgs_per_cu * cus / 8));
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <atomic>
#include <initializer_list>

// CU count of the current device (256 where it cannot be asked), asked once per device index
inline int lgx_cu_count() {
  constexpr int MAX_DEV = 64;
  static std::atomic<int> cached[MAX_DEV];   // 0: not asked yet
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess) return cus;
  const bool slot = dev >= 0 && dev < MAX_DEV;
  if (slot && cached[dev].load(std::memory_order_relaxed) > 0) return cached[dev].load(std::memory_order_relaxed);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 256;
  if (slot) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// Allow `bytes` of dynamic LDS (above the 64 KB default) for each of the n kernels; true when
// every hipFuncSetAttribute succeeded.  A caller keeps the result in a function-local static.
template <class Kernel>
bool lgx_allow_dynamic_lds(const Kernel* kernels, size_t n, int bytes) {
  bool ok = true;
  for (size_t i = 0; i < n; ++i)
    ok &= hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize,
                              bytes) == hipSuccess;
  return ok;
}
template <class Kernel>
bool lgx_allow_dynamic_lds(std::initializer_list<Kernel> kernels, int bytes) {
  return lgx_allow_dynamic_lds(kernels.begin(), kernels.size(), bytes);
}
#endif
