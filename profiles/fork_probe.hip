// fork_probe.hip -- the two open choices of copy_rows_kernel (csrc/pic_copy.h) measured on bare buffers: plain against
// write-through stores, and which grid dimension walks the environments (profiles/fork.md).  Identity copy and a broadcast of
// row 0, x and v in one launch as pic_copy_envs makes it, at config 2's shape (64 x 1e6 float64) and the reference's (256 x 5000).
//
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -Ioptimal-control-1d-electrostatic-plasma_amd/csrc
//         profiles/fork_probe.hip -o profiles/bin/fork_probe && profiles/bin/fork_probe
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "pic_device.h"
#include "pic_copy.h"

#define CHECK(call)                                                                                  \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) { std::printf("%s: %s\n", #call, hipGetErrorString(e_)); return 1; }      \
  } while (0)

// copy_rows_kernel's loop with the two choices open: WT = write-through stores, ENV_FAST = blockIdx.x walks the environments.
// <true, true> is the library's kernel.
template <bool WT, bool ENV_FAST>
__global__ __launch_bounds__(kCopyBlock) void probe_rows_kernel(const CopyRowsArgs g) {
  const int e = ENV_FAST ? (int)blockIdx.x : (int)blockIdx.y;
  const long long c0 = ENV_FAST ? blockIdx.y : blockIdx.x;
  const long long cstep = ENV_FAST ? gridDim.y : gridDim.x;
  const int m = copy_source(g.map, e, g.E_src, g.same);
  if (m < 0) return;
  const CopyRowSet r = blockIdx.z == 0 ? g.a[0] : g.a[1];
  const pic_v4u* src = reinterpret_cast<const pic_v4u*>(r.src + (size_t)m * r.src_stride);
  char* dst = r.dst + (size_t)e * r.dst_stride;
  constexpr long long kRound = (long long)kCopyBlock * kCopyUnroll;
  const long long last = r.nvec - 1;
  for (long long base = c0 * kRound; base < r.nvec; base += cstep * kRound) {
    pic_v4u w[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) {
      const long long i = base + u * kCopyBlock + threadIdx.x;
      w[u] = src[i < last ? i : last];
    }
    char* out = dst + base * 16;
    const StreamOut so(out);
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) {
      const int off = (u * kCopyBlock + (int)threadIdx.x) * 16;
      if (base + u * kCopyBlock + threadIdx.x <= last) {
        if (WT) so.store(off, w[u]);
        else *reinterpret_cast<pic_v4u*>(out + off) = w[u];
      }
    }
  }
}

template <bool WT, bool ENV_FAST>
static void launch(const CopyRowsArgs& a, int E, long long nvec, hipStream_t s) {
  const long long round = (long long)kCopyBlock * kCopyUnroll;
  const unsigned chunks = (unsigned)std::min<long long>((nvec + round - 1) / round, 65535);
  const dim3 grid = ENV_FAST ? dim3(E, chunks, 2) : dim3(chunks, E, 2);
  hipLaunchKernelGGL((probe_rows_kernel<WT, ENV_FAST>), grid, dim3(kCopyBlock), 0, s, a);
}

int main() {
  hipStream_t s;
  CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const struct { int E; long long ld; } shapes[2] = {{64, 1000000}, {256, 5056}};
  for (const auto& sh : shapes) {
    const long long row = sh.ld * 8;
    const size_t bytes = (size_t)sh.E * row;
    char *sx, *sv, *dx, *dv;
    int* zeros;
    CHECK(hipMalloc(&sx, bytes)); CHECK(hipMalloc(&sv, bytes)); CHECK(hipMalloc(&dx, bytes)); CHECK(hipMalloc(&dv, bytes));
    CHECK(hipMalloc(&zeros, sh.E * sizeof(int)));
    CHECK(hipMemset(sx, 1, bytes)); CHECK(hipMemset(sv, 2, bytes)); CHECK(hipMemset(dx, 0, bytes)); CHECK(hipMemset(dv, 0, bytes));
    CHECK(hipMemset(zeros, 0, sh.E * sizeof(int)));
    const int reps = 10;
    for (int bcast = 0; bcast < 2; ++bcast)
      for (int wt = 0; wt < 2; ++wt)
        for (int fast = 0; fast < 2; ++fast) {
          CopyRowsArgs a{};
          a.a[0] = CopyRowSet{sx, dx, row, row, row / 16};
          a.a[1] = CopyRowSet{sv, dv, row, row, row / 16};
          a.map = bcast ? zeros : nullptr; a.E_src = sh.E; a.same = 0;
          float best = 1e30f, sum = 0.f;
          for (int r = 0; r < reps + 2; ++r) {
            CHECK(hipEventRecord(e0, s));
            const long long nv = row / 16;
            if (wt) { if (fast) launch<true, true>(a, sh.E, nv, s); else launch<true, false>(a, sh.E, nv, s); }
            else { if (fast) launch<false, true>(a, sh.E, nv, s); else launch<false, false>(a, sh.E, nv, s); }
            CHECK(hipEventRecord(e1, s));
            CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 2) { best = std::min(best, ms); sum += ms; }
          }
          const double written = 2.0 * bytes, moved = bcast ? written : 2.0 * written;
          std::printf("E=%d ld=%lld %s stores=%s walk=%s  mean %.1f us  best %.1f us  (%.0f GB/s written, %.0f GB/s read+written)\n",
                      sh.E, sh.ld, bcast ? "broadcast" : "identity ", wt ? "write-through" : "plain        ",
                      fast ? "env-fast  " : "chunk-fast", sum / reps * 1e3, best * 1e3, written / (sum / reps * 1e-3) / 1e9,
                      moved / (sum / reps * 1e-3) / 1e9);
        }
    {                                   // the runtime's own device-to-device copy of the same bytes
      float sum = 0.f;
      for (int r = 0; r < reps + 2; ++r) {
        CHECK(hipEventRecord(e0, s));
        CHECK(hipMemcpyAsync(dx, sx, bytes, hipMemcpyDeviceToDevice, s));
        CHECK(hipMemcpyAsync(dv, sv, bytes, hipMemcpyDeviceToDevice, s));
        CHECK(hipEventRecord(e1, s));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) sum += ms;
      }
      std::printf("E=%d ld=%lld hipMemcpyAsync x2  mean %.1f us  (%.0f GB/s read+written)\n", sh.E, sh.ld, sum / reps * 1e3,
                  4.0 * bytes / (sum / reps * 1e-3) / 1e9);
    }
    // (a check of the last variant's result: every destination byte is its source's)
    std::vector<char> h(4096);
    CHECK(hipMemcpy(h.data(), dx + bytes - 4096, 4096, hipMemcpyDeviceToHost));
    for (char c : h) if (c != 1) { std::printf("copy check failed\n"); return 1; }
    hipFree(sx); hipFree(sv); hipFree(dx); hipFree(dv); hipFree(zeros);
  }
  return 0;
}
