// Micro-benchmark: rate of fire-and-forget global fp32 atomics on MI355X for different
// address patterns (used to decide how a symmetric half-stencil SpMV may write its
// transposed contributions).  hipcc --offload-arch=gfx950 -O3 atomic_ubench.hip -o atomic_ubench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

// pattern 0: lane l of global thread t adds to y[(t*rep + r) % n]   -> fully coalesced waves (64 consecutive floats)
// pattern 1: each thread owns 4 consecutive rows (stride-4 lanes)    -> 4 atomics, lanes 16 B apart
// pattern 2: random rows
// pattern 3: coalesced, but windows of neighbouring blocks overlap by 25% (contention between blocks)
// pattern 5: staged tap records -- a wave instruction adds into 4 runs of 64 bytes (4 records of 16 bytes, floats 0..2 of each;
//            lanes with l & 3 == 3 idle: 48 active lanes of 64), every run at its own random 16-byte aligned start
__global__ __launch_bounds__(256) void k_atomic(float* __restrict__ y, int n, int per_thread, int pattern, float v) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (pattern == 0) {
    for (int r = 0; r < per_thread; ++r) {
      int j = (int)(((long long)r * gridDim.x * blockDim.x + t) % n);
      unsafeAtomicAdd(y + j, v);
    }
  } else if (pattern == 1) {
    for (int r = 0; r < per_thread; r += 4) {
      long long b = ((long long)(r / 4) * gridDim.x * blockDim.x + t) * 4 % n;
#pragma unroll
      for (int e = 0; e < 4; ++e) unsafeAtomicAdd(y + b + e, v);
    }
  } else if (pattern == 2) {
    unsigned s = t * 2654435761u + 12345u;
    for (int r = 0; r < per_thread; ++r) {
      s = s * 1664525u + 1013904223u;
      unsafeAtomicAdd(y + (s >> 8) % n, v);
    }
  } else if (pattern == 3) {
    for (int r = 0; r < per_thread; ++r) {
      long long j = ((long long)r * gridDim.x + blockIdx.x) * 192 + threadIdx.x;
      unsafeAtomicAdd(y + j % n, v);
    }
  } else if (pattern == 5) {
    const int l = threadIdx.x & 63;
    const unsigned nrec = (unsigned)n / 4;                                      // n: a multiple of 4, >= 16
    unsigned s = (unsigned)(t >> 6) * 2654435761u + 12345u;                     // wave-uniform
    for (int r = 0; r < per_thread; ++r) {
      s = s * 1664525u + 1013904223u;
      const unsigned h = (s ^ ((unsigned)(l >> 4) * 0x9E3779B9u)) * 2246822519u;  // one start per run of 16 lanes
      const unsigned rec = (h >> 8) % (nrec - 3) + (unsigned)((l >> 2) & 3);      // <= nrec - 1
      if ((l & 3) != 3) unsafeAtomicAdd(y + (size_t)rec * 4 + (l & 3), v);
    }
  } else if (pattern == 4) {   // plain coalesced read-modify-write (no atomic) for reference
    for (int r = 0; r < per_thread; ++r) {
      int j = (int)(((long long)r * gridDim.x * blockDim.x + t) % n);
      y[j] += v;
    }
  }
}

int main() {
  const int n = 1 << 21;   // 8 MB target
  float* y;
  hipMalloc(&y, (size_t)n * 4);
  hipMemset(y, 0, (size_t)n * 4);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const char* names[] = {"coalesced", "4-row threads", "random", "coalesced, overlapping blocks", "plain RMW (no atomic)"};
  for (int target : {1 << 17, 1 << 21}) {
    for (int pattern = 0; pattern < 5; ++pattern) {
      for (int blocks : {512, 2048}) {
        const int per_thread = 16;
        hipLaunchKernelGGL(k_atomic, dim3(blocks), dim3(256), 0, 0, y, target, per_thread, pattern, 1.0f);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        const int reps = 20;
        for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_atomic, dim3(blocks), dim3(256), 0, 0, y, target, per_thread, pattern, 1.0f);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        const double ops = (double)blocks * 256 * per_thread * reps;
        printf("target %7d floats  %-32s blocks %4d : %8.2f us/launch  %7.1f G lane-atomics/s\n", target, names[pattern], blocks, ms * 1e3 / reps,
               ops / (ms * 1e-3) / 1e9);
      }
    }
  }
  // the staged-record shape of a node-major {b, cnt, res, -} buffer (2 MB = 125 000 nodes) beside the 16-byte runs of one of the
  // three [m] arrays (0.5 MB), counted in ACTIVE lanes
  for (int pattern : {1, 5}) {
    const int target = pattern == 1 ? 1 << 17 : 1 << 19;
    for (int blocks : {512, 2048}) {
      const int per_thread = 16;
      hipLaunchKernelGGL(k_atomic, dim3(blocks), dim3(256), 0, 0, y, target, per_thread, pattern, 1.0f);
      hipDeviceSynchronize();
      hipEventRecord(e0);
      const int reps = 20;
      for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_atomic, dim3(blocks), dim3(256), 0, 0, y, target, per_thread, pattern, 1.0f);
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      const double ops = (double)blocks * 256 * per_thread * reps * (pattern == 5 ? 0.75 : 1.0);
      printf("target %7d floats  %-32s blocks %4d : %8.2f us/launch  %7.1f G active lane-atomics/s\n", target,
             pattern == 1 ? "4-row threads (16-byte runs)" : "staged records (64-byte runs)", blocks, ms * 1e3 / reps, ops / (ms * 1e-3) / 1e9);
    }
  }
  return 0;
}
