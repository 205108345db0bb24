// pic_copy.h -- copies of whole environments on the device (pic_copy_envs): environment e of the destination
// becomes environment map[e] of the source, inside one handle (fork) or between two (broadcast / restore).
//
//   copy_rows_kernel        the particle rows x, v (and the resident schedule's carried cells) as bytes: rows with a per-row
//                           source index, 16 bytes per lane, kCopyUnroll loads in flight per lane before the first store
//   copy_env_small_kernel   one workgroup per destination environment: meshes, energies, the cached deposit's sub-rows, the
//                           resident q1 mesh; it also counts the map entries a device map gets wrong
//
// Both read the map entry of their environment themselves (wave-uniform: a scalar load) and check it before any address is
// formed from it: an entry out of range, or one that breaks the keep rule of a fork, copies nothing.
#pragma once

namespace {

constexpr int kCopyBlock = 256;      // threads of a copy workgroup
constexpr int kCopyUnroll = 8;       // 16-byte loads a lane has in flight: 32 KB per workgroup and round
constexpr int kCopyArrays = 3;       // x, v, carried cells
constexpr int kCopySegments = 8;     // n, E_mesh, phi, KE, PE, PE_reward, deposit row, resident q1 mesh

// one array of rows: row e of dst <- row map[e] of src.  Strides in bytes; nvec: 16-byte vectors of a row
struct CopyRowSet {
  const char* src;
  char* dst;
  long long src_stride, dst_stride;
  long long nvec;
};

struct CopyRowsArgs {
  CopyRowSet a[kCopyArrays];         // blockIdx.z picks one
  const int* map;                    // [E_dst] device memory, or null: identity
  int E_src;
  int same;                          // source and destination are one handle: kept rows are skipped, sources must be kept rows
};

// words of 8 bytes: for sub in [0, nsub), j in [0, n): dst[e dst_env + sub dst_sub + j] <- src[m src_env + sub src_sub + j]
struct CopySeg {
  const unsigned long long* src;
  unsigned long long* dst;
  long long src_env, dst_env, src_sub, dst_sub;
  int n, nsub;                       // n = 0: unused
};

struct CopySmallArgs {
  CopySeg s[kCopySegments];
  const int* map;
  int E_src;
  int same;
  unsigned long long* rejected;      // + 1 per environment whose entry is refused
};

enum : int { kCopyRejected = -1, kCopyKept = -2 };

// the source environment of destination e, kCopyKept (a fork keeps e) or kCopyRejected.  map[m] is read only for 0 <= m < E_src
// (same handle: E_src entries exist).
__device__ __forceinline__ int copy_source(const int* map, int e, int E_src, int same) {
  const int m = map ? map[e] : e;
  if ((unsigned)m >= (unsigned)E_src) return kCopyRejected;
  if (same) {
    if (m == e) return kCopyKept;
    if (map[m] != m) return kCopyRejected;
  }
  return m;
}

// Grid (environments, chunks, arrays): blockIdx.x walks the environments, so the workgroups of one source chunk are neighbours in
// launch order and a broadcast reads the chunk from memory once.  Stores are plain: unlike behind a sweep (pic_device.h:
// StreamOut), the step behind a copy takes the same time after plain and after write-through stores, and the broadcast itself
// is 9 % faster with plain ones at 64 x 1e6.  Both choices were measured against their alternatives (profiles/fork.md; the
// variants on bare buffers live in profiles/fork_probe.hip).  PIC_COPY_WRITE_THROUGH=1 builds the write-through kernel for
// profiles/fork.py --write-through, which times the step behind it; the library is never built that way.
// Every load of a round is issued before its first store and none sits under a branch: a lane past the end of the row loads the
// row's last vector again and stores nothing (rows are multiples of 64 elements, so a row has whole vectors only; the last round
// of a row may have idle lanes).
#ifndef PIC_COPY_WRITE_THROUGH
#define PIC_COPY_WRITE_THROUGH 0
#endif
__global__ __launch_bounds__(kCopyBlock) void copy_rows_kernel(const CopyRowsArgs g) {
  const int e = blockIdx.x;
  const long long c0 = blockIdx.y;
  const long long cstep = gridDim.y;
  const int m = copy_source(g.map, e, g.E_src, g.same);
  if (m < 0) return;
  const int z = blockIdx.z;
  const CopyRowSet r = z == 0 ? g.a[0] : (z == 1 ? g.a[1] : g.a[2]);
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
    char* out = dst + base * 16;                     // wave-uniform; a round is 32 KB
    const StreamOut so(out);
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) {
      const int off = (u * kCopyBlock + (int)threadIdx.x) * 16;
      if (base + u * kCopyBlock + threadIdx.x <= last) {
        if (PIC_COPY_WRITE_THROUGH) so.store(off, w[u]);
        else *reinterpret_cast<pic_v4u*>(out + off) = w[u];
      }
    }
  }
}

__global__ __launch_bounds__(kCopyBlock) void copy_env_small_kernel(const CopySmallArgs g) {
  const int e = blockIdx.x;
  const int m = copy_source(g.map, e, g.E_src, g.same);
  if (m == kCopyRejected) {
    if (threadIdx.x == 0) atomicAdd(g.rejected, 1ull);
    return;
  }
  if (m < 0) return;
#pragma unroll
  for (int k = 0; k < kCopySegments; ++k) {
    const CopySeg s = g.s[k];
    const unsigned long long* src = s.src + (size_t)m * s.src_env;
    unsigned long long* dst = s.dst + (size_t)e * s.dst_env;
    const int total = s.n * s.nsub;
    for (int i = threadIdx.x; i < total; i += kCopyBlock) {
      const int sub = i / s.n, j = i - sub * s.n;
      dst[sub * s.dst_sub + j] = src[sub * s.src_sub + j];
    }
  }
}

}  // namespace
