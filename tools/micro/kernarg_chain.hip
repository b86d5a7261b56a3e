// kernarg_chain.hip — what one serialized scalar load from the kernel-argument
// segment costs a K2 wave (DevWorkload is read in place there: every field is
// an s_load in front of its use, waited for on the spot).  A grid of 1,500
// one-wave blocks in a fresh launch, as C3's K2: each wave does kLoads s_load
// + s_waitcnt pairs 128 bytes apart in a 2 KB argument block (a 64-byte
// scalar-cache line each) and
// times them with s_memtime, then the same lines again (scalar-cache hits).
// Build: hipcc -O3 --offload-arch=gfx950 -o kernarg_chain kernarg_chain.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int kLoads = 16;    // serialized loads per pass
constexpr int kStride = 128;  // bytes between them: a scalar-cache line each
constexpr int kWaves = 1500;

struct Args {
  uint32_t word[kLoads * kStride / 4];
};

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int I>
__device__ __forceinline__ uint32_t chain(const void* base, uint32_t acc) {
  if constexpr (I < kLoads) {
    uint32_t v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(base), "n"(I * kStride) : "memory");
    return chain<I + 1>(base, acc + v);
  } else {
    return acc;
  }
}
#pragma clang diagnostic pop

__global__ __launch_bounds__(64) void chain_kernel(Args a, uint32_t* out) {
  (void)a;
  const void* base = (const void*)__builtin_amdgcn_kernarg_segment_ptr();
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  uint32_t acc = chain<0>(base, 0);
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  acc = chain<0>(base, acc);
  const uint64_t t2 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x + 0] = static_cast<uint32_t>(t1 - t0);
    out[3 * blockIdx.x + 1] = static_cast<uint32_t>(t2 - t1);
    out[3 * blockIdx.x + 2] = acc;
  }
}

// a launch between two measurements: the measured one starts on cold scalar caches
__global__ void spacer_kernel(uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = 0;
}

int main() {
  Args a;
  for (size_t i = 0; i < sizeof(a.word) / 4; ++i) a.word[i] = static_cast<uint32_t>(i);
  uint32_t* out;
  if (hipMalloc(&out, kWaves * 3 * 4) != hipSuccess) return 1;
  std::vector<uint32_t> h(kWaves * 3);
  std::vector<double> first, repeat, first_max;
  for (int r = 0; r < 21; ++r) {
    a.word[0] = static_cast<uint32_t>(r);  // new argument contents every launch
    spacer_kernel<<<(kWaves * 3 + 255) / 256, 256>>>(out, kWaves * 3);
    chain_kernel<<<kWaves, 64>>>(a, out);
    if (hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    std::vector<uint32_t> f(kWaves), s(kWaves);
    for (int i = 0; i < kWaves; ++i) {
      f[i] = h[3 * i];
      s[i] = h[3 * i + 1];
    }
    std::sort(f.begin(), f.end());
    std::sort(s.begin(), s.end());
    first.push_back(double(f[kWaves / 2]) / kLoads);
    first_max.push_back(double(f[kWaves - 1]) / kLoads);
    repeat.push_back(double(s[kWaves / 2]) / kLoads);
  }
  std::sort(first.begin(), first.end());
  std::sort(first_max.begin(), first_max.end());
  std::sort(repeat.begin(), repeat.end());
  printf("serialized kernel-argument s_load, %d waves, %d loads per pass (median of 21 launches)\n", kWaves, kLoads);
  printf("  first touch: %.0f cycles per load (median wave), %.0f (slowest wave)\n", first[10], first_max[10]);
  printf("  repeat (scalar-cache hit): %.0f cycles per load (median wave)\n", repeat[10]);
  return 0;
}
