// BitTorrent v2 (BEP 52) merkle hashing on the MI355X (gfx950).
//
// BEP 52 hashes every 16 KiB block of a file on its own (SHA-256), then pairs of digests up to
// the piece layer and on to the file's `pieces root`. Unlike the v1 SHA-1 arm (gpu_sha1.hip:
// one lane per piece, a few hundred lanes per launch) the unit of parallelism here is the
// block, whatever the piece length: a 1 GiB batch is 65,536 independent leaves - one wave on
// every SIMD of the chip - and the expensive part needs no cross-lane cooperation.
//
//   * sha256_leaves: ONE LANE PER 16 KiB BLOCK. Lane i streams data + i * 16384 with the
//     access pattern of sha1_run16: four dwordx4 loads per 64-byte block, block k+1 loaded
//     into a second register buffer while block k is hashed, the prefetch of the last pair
//     clamped to the lane's last block (always in bounds, no branch). Leaves are 16 KiB
//     aligned in the staging buffer, so only the 16-byte load path exists. Only the last leaf
//     of a file may be short (1 .. 16384 bytes, hashed at its true length).
//   * sha256_pairs: one lane per parent, message = the 64 bytes of its two children plus the
//     fixed padding block of a 512-bit message. Launched once per tree level on the batch's
//     stream, ping-ponging between two digest buffers; a level is tens of microseconds
//     against the milliseconds of the batch's DMA, so the levels are not fused.
//   * Digests live in device memory as the 32 digest bytes in SHA-256 output order, so the
//     next level reads them as message bytes.
//   * MerkleHasher double-buffers like GpuVerifier: two pinned staging slots, two streams;
//     reader threads fill slot s while the other slot's copy and kernels run. A batch is a
//     whole number of pieces; the digest region of a file's last piece is zero-filled up to
//     the leaves-per-piece count before reduction (a missing leaf is 32 zero bytes), so every
//     level halves uniformly. The piece layer is reduced to the root on the device too, padded
//     to a power of two with the pad hash of its level.
//   * hash_files / verify_files take a whole torrent's files: a batch holds units (pieces, or
//     whole small files) of many files at once, laid out by merkle_plan.h so that ONE
//     sha256_leaf_table launch (one lane per leaf-table entry) and ONE sha256_pairs_fin launch
//     per level reduce subtrees of different heights together; the batch loop drains a slot
//     only when it comes round again, so fills and device work overlap across files.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <exception>
#include <fcntl.h>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "merkle_plan.h"

namespace py = pybind11;
namespace mp = stager::merkle_plan;

// A failed call stays behind as the thread's "last error" until hipGetLastError() reads it, and
// every launch here is checked with hipGetLastError(): the error is taken off the thread as it
// is reported, so it does not come back from the next launch.
#define HIP_CHECK(x)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      (void)hipGetLastError();                                                            \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " + \
                               #x);                                                       \
    }                                                                                     \
  } while (0)

namespace {

constexpr int64_t kLeaf = 16384;  // BEP 52 block size
static_assert(kLeaf == mp::kLeaf, "the plan and the kernels share the block size");

using PlanLeaf = mp::Leaf;  // one lane of sha256_leaf_table reads its entry as one 16-byte load
static_assert(sizeof(PlanLeaf) == 16 && alignof(PlanLeaf) == 8, "leaf table entry layout");

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) {
  return __builtin_amdgcn_alignbit(x, x, n);
}
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// gfx950 V_BITOP3_B32: any 3-input bitwise function in one VALU op, selected by an 8-bit truth
// table. Only symmetric tables are used (operand order cannot matter): 0x96 = a ^ b ^ c (the
// four sigma functions), 0xE8 = majority(a, b, c). hipcc does not form these from plain C.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ uint32_t maj(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xe8" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ uint32_t ch(uint32_t e, uint32_t f, uint32_t g) {
  // Plain C: the two terms are disjoint, so hipcc emits v_and + v_bitop3 (g & ~e) and folds
  // the OR into the v_add3 chain of the round (no separate v_bfi_b32 / v_or).
  return (e & f) | (~e & g);
}
__device__ __forceinline__ uint32_t bsig0(uint32_t x) { return xor3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
__device__ __forceinline__ uint32_t bsig1(uint32_t x) { return xor3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
__device__ __forceinline__ uint32_t ssig0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
__device__ __forceinline__ uint32_t ssig1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }

struct Sha256State {
  uint32_t h[8];
};

__device__ __forceinline__ void sha256_init(Sha256State& s) {
  s.h[0] = 0x6a09e667u;
  s.h[1] = 0xbb67ae85u;
  s.h[2] = 0x3c6ef372u;
  s.h[3] = 0xa54ff53au;
  s.h[4] = 0x510e527fu;
  s.h[5] = 0x9b05688cu;
  s.h[6] = 0x1f83d9abu;
  s.h[7] = 0x5be0cd19u;
}

// One round with the working variables named in place (the caller rotates the names, so no
// register moves), `t` and `K` literals: the schedule branch folds and K is an inline constant.
#define S256_ROUND(a, b, c, d, e, f, g, h, t, K)                                          \
  {                                                                                       \
    if ((t) >= 16)                                                                        \
      w[(t)&15] += ssig1(w[((t)-2) & 15]) + w[((t)-7) & 15] + ssig0(w[((t)-15) & 15]);    \
    const uint32_t t1 = h + bsig1(e) + ch(e, f, g) + (K) + w[(t)&15];                     \
    const uint32_t t2 = bsig0(a) + maj(a, b, c);                                          \
    d += t1;                                                                              \
    h = t1 + t2;                                                                          \
  }
#define S256_ROUND8(t, K0, K1, K2, K3, K4, K5, K6, K7) \
  S256_ROUND(a, b, c, d, e, f, g, h, (t) + 0, K0)      \
  S256_ROUND(h, a, b, c, d, e, f, g, (t) + 1, K1)      \
  S256_ROUND(g, h, a, b, c, d, e, f, (t) + 2, K2)      \
  S256_ROUND(f, g, h, a, b, c, d, e, (t) + 3, K3)      \
  S256_ROUND(e, f, g, h, a, b, c, d, (t) + 4, K4)      \
  S256_ROUND(d, e, f, g, h, a, b, c, (t) + 5, K5)      \
  S256_ROUND(c, d, e, f, g, h, a, b, (t) + 6, K6)      \
  S256_ROUND(b, c, d, e, f, g, h, a, (t) + 7, K7)

// 64 rounds, fully unrolled; w[] is the rolling 16-word schedule and is consumed.
__device__ __forceinline__ void sha256_block(Sha256State& s, uint32_t w[16]) {
  uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3];
  uint32_t e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
  S256_ROUND8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u,
              0x923f82a4u, 0xab1c5ed5u)
  S256_ROUND8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,
              0x9bdc06a7u, 0xc19bf174u)
  S256_ROUND8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
              0x5cb0a9dcu, 0x76f988dau)
  S256_ROUND8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
              0x06ca6351u, 0x14292967u)
  S256_ROUND8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu,
              0x81c2c92eu, 0x92722c85u)
  S256_ROUND8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u,
              0xf40e3585u, 0x106aa070u)
  S256_ROUND8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au,
              0x5b9cca4fu, 0x682e6ff3u)
  S256_ROUND8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu,
              0xbef9a3f7u, 0xc67178f2u)
  s.h[0] += a;
  s.h[1] += b;
  s.h[2] += c;
  s.h[3] += d;
  s.h[4] += e;
  s.h[5] += f;
  s.h[6] += g;
  s.h[7] += h;
}

// Raw 64-byte block as four dwordx4 loads, and its conversion to big-endian words: split so
// the loads of block k+1 can be issued before block k is hashed.
__device__ __forceinline__ void load_raw16(const uint8_t* p, uint4 v[4]) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = q[i];
}
__device__ __forceinline__ void to_words(const uint4 v[4], uint32_t w[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[4 * i + 0] = bswap(v[i].x);
    w[4 * i + 1] = bswap(v[i].y);
    w[4 * i + 2] = bswap(v[i].z);
    w[4 * i + 3] = bswap(v[i].w);
  }
}

// `nblk` whole blocks at p (16-byte aligned) into s. Two register buffers with fixed roles (no
// cur = nxt copy: a move out of a register with a load in flight waits for that load). The
// second load of a pair is clamped to the lane's last whole block, so it never leaves
// [p, p + 64 * nblk); the duplicate 64 bytes are never hashed.
__device__ __forceinline__ void sha256_run16(Sha256State& s, const uint8_t* p, int nblk) {
  if (nblk <= 0) return;
  uint32_t w[16];
  uint4 a[4], b[4];
  load_raw16(p, a);
  int blk = 0;
  for (; blk + 2 <= nblk; blk += 2) {
    load_raw16(p + ((int64_t)(blk + 1) << 6), b);
    to_words(a, w);
    sha256_block(s, w);
    const int n2 = blk + 2 < nblk ? blk + 2 : nblk - 1;
    load_raw16(p + ((int64_t)n2 << 6), a);
    to_words(b, w);
    sha256_block(s, w);
  }
  if (blk < nblk) {
    to_words(a, w);
    sha256_block(s, w);
  }
}

// The 32 digest bytes in SHA-256 output order, as two 16-byte vector stores (o is 32-byte
// aligned: digest buffers are hipMalloc'ed and indexed in units of 32).
__device__ __forceinline__ void store_digest(uint8_t* o, const Sha256State& s) {
  uint4* q = reinterpret_cast<uint4*>(o);
  q[0] = make_uint4(bswap(s.h[0]), bswap(s.h[1]), bswap(s.h[2]), bswap(s.h[3]));
  q[1] = make_uint4(bswap(s.h[4]), bswap(s.h[5]), bswap(s.h[6]), bswap(s.h[7]));
}

// One leaf: SHA-256 of the `len` bytes (1 .. 16384) at p (16-byte aligned), digest to o. Whole
// blocks, then tail + padding built word by word into w[]: a remainder of 56 bytes or more
// takes two padding blocks, a remainder of 0 (every full leaf) one whole padding block. Tail
// bytes are read one by one and only below `rem`: nothing at or past p + len is touched.
__device__ __forceinline__ void sha256_leaf(const uint8_t* __restrict__ p, int len,
                                            uint8_t* __restrict__ o) {
  Sha256State s;
  sha256_init(s);
  const int nfull = len >> 6;
  sha256_run16(s, p, nfull);
  uint32_t w[16];
  const int rem = len & 63;
  const uint8_t* tail = p + ((int64_t)nfull << 6);
  const uint64_t bits = (uint64_t)len * 8ull;
  const int nb = rem >= 56 ? 2 : 1;
  for (int b = 0; b < nb; ++b) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = b * 64 + 4 * k + j;
        const uint32_t byte = idx < rem ? (uint32_t)tail[idx] : (idx == rem ? 0x80u : 0u);
        v |= byte << (24 - 8 * j);
      }
      w[k] = v;
    }
    if (b == nb - 1) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    sha256_block(s, w);
  }
  store_digest(o, s);
}

// Lane i: the 16 KiB block at data + i * 16384 (the last lane: last_len bytes, 1 .. 16384),
// digest to out + 32 * i.
__global__ __launch_bounds__(64) void sha256_leaves(const uint8_t* __restrict__ data,
                                                    int64_t n_leaves, int last_len,
                                                    uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_leaves) return;
  const int len = (i == n_leaves - 1) ? last_len : (int)kLeaf;
  sha256_leaf(data + i * kLeaf, len, out + i * 32);
}

// Lane i: leaf i of a batch plan's leaf table (merkle_plan.h): table[i].len bytes at
// data + table[i].src, digest to out + 32 * table[i].dst. The slot holds pieces of many files;
// the bytes between two files are stale data of an earlier batch and no lane reads them.
__global__ __launch_bounds__(64) void sha256_leaf_table(const uint8_t* __restrict__ data,
                                                        const PlanLeaf* __restrict__ table,
                                                        int64_t n_leaves,
                                                        uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_leaves) return;
  const PlanLeaf e = table[i];
  sha256_leaf(data + e.src, e.len, out + (int64_t)e.dst * 32);
}

// SHA-256 of the 64 bytes at p (two child digests).
__device__ __forceinline__ void sha256_pair(Sha256State& s, const uint8_t* __restrict__ p) {
  sha256_init(s);
  uint4 v[4];
  uint32_t w[16];
  load_raw16(p, v);
  to_words(v, w);
  sha256_block(s, w);
  w[0] = 0x80000000u;  // the padding block of a 512-bit message
#pragma unroll
  for (int k = 1; k < 15; ++k) w[k] = 0;
  w[15] = 512u;
  sha256_block(s, w);
}

// Lane i: SHA-256 of the 64 bytes at in + 64 * i (two child digests) -> out + 32 * i.
__global__ __launch_bounds__(64) void sha256_pairs(const uint8_t* __restrict__ in, int64_t n,
                                                   uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Sha256State s;
  sha256_pair(s, in + i * 64);
  store_digest(out + i * 32, s);
}

// One level of a batch plan: sha256_pairs over the units still being reduced, and the outputs
// from fin_start on are finished unit nodes, written to result + 32 * (unit_base + i -
// fin_start) as well (the sorted unit order of merkle_plan.h).
__global__ __launch_bounds__(64) void sha256_pairs_fin(const uint8_t* __restrict__ in, int64_t n,
                                                       uint8_t* __restrict__ out,
                                                       int64_t fin_start, int64_t unit_base,
                                                       uint8_t* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Sha256State s;
  sha256_pair(s, in + i * 64);
  store_digest(out + i * 32, s);
  if (i >= fin_start) store_digest(result + (unit_base + i - fin_start) * 32, s);
}

void launch_leaves(hipStream_t st, const uint8_t* d_data, int64_t n, int last_len, uint8_t* d_out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sha256_leaves, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_data, n,
                     last_len, d_out);
  HIP_CHECK(hipGetLastError());
}

void launch_pairs(hipStream_t st, const uint8_t* d_in, int64_t n, uint8_t* d_out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sha256_pairs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_in, n,
                     d_out);
  HIP_CHECK(hipGetLastError());
}

void launch_leaf_table(hipStream_t st, const uint8_t* d_data, const PlanLeaf* d_table, int64_t n,
                       uint8_t* d_out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sha256_leaf_table, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_data,
                     d_table, n, d_out);
  HIP_CHECK(hipGetLastError());
}

void launch_pairs_fin(hipStream_t st, const uint8_t* d_in, const mp::Level& lv, uint8_t* d_out,
                      uint8_t* d_result) {
  if (lv.n_pairs <= 0) return;
  hipLaunchKernelGGL(sha256_pairs_fin, dim3((unsigned)((lv.n_pairs + 63) / 64)), dim3(64), 0, st,
                     d_in, lv.n_pairs, d_out, lv.fin_start, lv.unit_base, d_result);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
template <class F>
void parallel_for(size_t n, int threads, F&& fn) {
  threads = std::max(1, std::min<int>(threads, (int)n));
  if (threads == 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  // An exception in a reader (or a thread that cannot be started) reaches the caller instead
  // of std::terminate: the first one is rethrown once every started thread has joined.
  std::atomic<size_t> next{0};
  std::mutex err_mu;
  std::exception_ptr err;
  auto work = [&] {
    try {
      for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
    } catch (...) {
      next.store(n);
      std::lock_guard<std::mutex> g(err_mu);
      if (!err) err = std::current_exception();
    }
  };
  std::vector<std::thread> pool;
  try {
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  } catch (...) {
    // fewer threads than asked: the ones running (and this one) share the work
  }
  work();
  for (auto& th : pool) th.join();
  if (err) std::rethrow_exception(err);
}

// Scoped device memory and events: released on every exit path, a thrown HIP error included.
template <class T>
struct DevMem {
  T* p = nullptr;
  explicit DevMem(size_t n) {
    if (n) HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
  }
  ~DevMem() {
    if (p) hipFree(p);
  }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
};
struct DevEvent {
  hipEvent_t e = nullptr;
  explicit DevEvent(unsigned flags = hipEventDisableTiming) {
    HIP_CHECK(hipEventCreateWithFlags(&e, flags));
  }
  ~DevEvent() {
    if (e) hipEventDestroy(e);
  }
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
};

struct Fd {
  int fd;
  explicit Fd(const std::string& path) : fd(::open(path.c_str(), O_RDONLY | O_CLOEXEC)) {}
  ~Fd() {
    if (fd >= 0) ::close(fd);
  }
  Fd(const Fd&) = delete;
  Fd& operator=(const Fd&) = delete;
};

bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
int64_t pow2_ceil(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
int log2_exact(int64_t v) {
  int k = 0;
  while (((int64_t)1 << k) < v) ++k;
  return k;
}

using Digest = std::array<uint8_t, 32>;
using FileList = std::vector<std::pair<std::string, int64_t>>;  // (path, length)

struct Tree {
  std::string layer;  // 32 bytes per piece; empty when the file is no larger than a piece
  std::string root;   // 32 bytes
};

class MerkleHasher {
  // A fill puts bytes [off, off + len) of the source at dst and returns how many leading
  // bytes it could deliver (len when all of them). Both split the range over reader threads.
  static constexpr int64_t kFillChunk = 1 << 20;

  auto buffer_fill(const uint8_t* p) {
    return [this, p](int64_t off, int64_t len, uint8_t* dst) -> int64_t {
      const size_t nch = (size_t)((len + kFillChunk - 1) / kFillChunk);
      parallel_for(nch, readers_, [&](size_t c) {
        const int64_t o = (int64_t)c * kFillChunk, n = std::min(kFillChunk, len - o);
        memcpy(dst + o, p + off + o, (size_t)n);
      });
      return len;
    };
  }

  auto file_fill(int fd) {
    return [this, fd](int64_t off, int64_t len, uint8_t* dst) -> int64_t {
      const size_t nch = (size_t)((len + kFillChunk - 1) / kFillChunk);
      std::atomic<int64_t> good{len};
      parallel_for(nch, readers_, [&](size_t c) {
        const int64_t o = (int64_t)c * kFillChunk, n = std::min(kFillChunk, len - o);
        int64_t got = 0;
        while (got < n) {
          ssize_t r = pread(fd, dst + o + got, (size_t)(n - got), off + o + got);
          if (r < 0 && errno == EINTR) continue;
          if (r <= 0) break;
          got += r;
        }
        if (got < n) {
          int64_t at = o + got, cur = good.load();
          while (at < cur && !good.compare_exchange_weak(cur, at)) {
          }
        }
      });
      return good.load();
    };
  }

 public:
  MerkleHasher(int device, int64_t batch_bytes, int reader_threads)
      : device_(device), batch_bytes_(batch_bytes), readers_(std::max(1, reader_threads)) {
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw std::runtime_error("no such HIP device");
    HIP_CHECK(hipSetDevice(device_));
    dig_bytes_ = (size_t)(batch_bytes_ / kLeaf) * 32;
    try {
      for (int s = 0; s < 2; ++s) {
        HIP_CHECK(hipStreamCreateWithFlags(&stream_[s], hipStreamNonBlocking));
        HIP_CHECK(hipHostMalloc((void**)&h_buf_[s], (size_t)batch_bytes_, hipHostMallocDefault));
        HIP_CHECK(hipMalloc((void**)&d_buf_[s], (size_t)batch_bytes_));
        HIP_CHECK(hipHostMalloc((void**)&h_dig_[s], dig_bytes_, hipHostMallocDefault));
        for (int b = 0; b < 2; ++b) HIP_CHECK(hipMalloc((void**)&d_dig_[s][b], dig_bytes_));
      }
    } catch (...) {
      release();  // a failed set-up leaves nothing allocated
      throw;
    }
    pads_.push_back(Digest{});  // pad_hash(0): 32 zero bytes
  }
  ~MerkleHasher() { release(); }
  MerkleHasher(const MerkleHasher&) = delete;
  MerkleHasher& operator=(const MerkleHasher&) = delete;

  int64_t batch_bytes() const { return batch_bytes_; }

  // pad_hash(0) = 32 zero bytes, pad_hash(k + 1) = sha256(pad_hash(k) * 2): the hash of an
  // all-missing subtree of 2^k leaves. Computed once per level with sha256_pairs.
  const Digest& pad_hash(int level) {
    if (level < 0 || level > 62) throw std::invalid_argument("pad_hash: level out of range");
    if ((size_t)level < pads_.size()) return pads_[(size_t)level];
    HIP_CHECK(hipSetDevice(device_));
    DevMem<uint8_t> in(64), out(32);
    while (pads_.size() <= (size_t)level) {
      uint8_t pair[64];
      memcpy(pair, pads_.back().data(), 32);
      memcpy(pair + 32, pads_.back().data(), 32);
      Digest d;
      HIP_CHECK(hipMemcpyAsync(in.p, pair, 64, hipMemcpyHostToDevice, stream_[0]));
      launch_pairs(stream_[0], in.p, 1, out.p);
      HIP_CHECK(hipMemcpyAsync(d.data(), out.p, 32, hipMemcpyDeviceToHost, stream_[0]));
      HIP_CHECK(hipStreamSynchronize(stream_[0]));
      pads_.push_back(d);
    }
    return pads_[(size_t)level];
  }

  // 32 bytes per 16 KiB block of a host buffer (the last block at its true length).
  std::string leaf_hashes(const uint8_t* p, int64_t n) {
    if (n == 0) return std::string();
    std::string out((size_t)((n + kLeaf - 1) / kLeaf) * 32, '\0');
    run(n, kLeaf, buffer_fill(p), (uint8_t*)out.data(), nullptr);
    return out;
  }

  // One level: `hashes` is k x 32 bytes, an odd k is completed with `pad`.
  std::string reduce_layer(const std::string& hashes, const std::string& pad) {
    const int64_t k = (int64_t)hashes.size() / 32, m = (k + 1) / 2;
    std::string in = hashes;
    if (k & 1) in += pad;
    std::string out((size_t)m * 32, '\0');
    HIP_CHECK(hipSetDevice(device_));
    DevMem<uint8_t> d_in(in.size()), d_out(out.size());
    HIP_CHECK(hipMemcpyAsync(d_in.p, in.data(), in.size(), hipMemcpyHostToDevice, stream_[0]));
    launch_pairs(stream_[0], d_in.p, m, d_out.p);
    HIP_CHECK(hipMemcpyAsync(&out[0], d_out.p, out.size(), hipMemcpyDeviceToHost, stream_[0]));
    HIP_CHECK(hipStreamSynchronize(stream_[0]));
    return out;
  }

  Tree hash_buffer(const uint8_t* p, int64_t n, int64_t piece_len) {
    return tree(n, piece_len, buffer_fill(p), nullptr);
  }

  Tree hash_file(const std::string& path, int64_t length, int64_t piece_len) {
    Fd f(path);
    if (f.fd < 0) throw std::runtime_error("cannot open " + path + ": " + strerror(errno));
    return tree(length, piece_len, file_fill(f.fd), nullptr);
  }

  // One byte per piece (1 = the piece's subtree hashes to `expected`'s node). A piece the
  // file on disk does not cover (missing or short file) is 0; its staging bytes are zeroed,
  // nothing is read past what pread returned.
  std::vector<uint8_t> verify_file(const std::string& path, int64_t length, int64_t piece_len,
                                   const std::string& expected) {
    const int64_t np = num_pieces(length, piece_len);
    std::vector<uint8_t> ok((size_t)np, 0);
    Fd f(path);
    if (f.fd < 0) return ok;
    std::vector<uint8_t> readable((size_t)np, 1);
    Tree t = tree(length, piece_len, file_fill(f.fd), readable.data(), /*want_root=*/false);
    const std::string& got = length > piece_len ? t.layer : t.root;
    for (int64_t i = 0; i < np; ++i)
      ok[(size_t)i] = readable[(size_t)i] &&
                      memcmp(got.data() + i * 32, expected.data() + i * 32, 32) == 0;
    return ok;
  }

  // 32 bytes per unit (merkle_plan.h: a piece of a file longer than piece_len, or a whole
  // smaller file), file order then piece order: the piece layers and the roots of the small
  // files, concatenated. A missing or short file is an error.
  std::string hash_files(const FileList& files, int64_t piece_len) {
    std::string out((size_t)total_units(files, piece_len) * 32, '\0');
    run_files(files, piece_len, (uint8_t*)out.data(), nullptr);
    return out;
  }

  // One byte per unit against `expected` (32 bytes per unit, the order of hash_files). A unit
  // its file on disk does not cover is 0; the other files of its batch are not affected.
  std::vector<uint8_t> verify_files(const FileList& files, int64_t piece_len,
                                    const std::string& expected) {
    const int64_t nu = total_units(files, piece_len);
    std::string got((size_t)nu * 32, '\0');
    std::vector<uint8_t> ok((size_t)nu, 1);
    run_files(files, piece_len, (uint8_t*)got.data(), ok.data());
    for (int64_t i = 0; i < nu; ++i)
      ok[(size_t)i] = ok[(size_t)i] &&
                      memcmp(got.data() + i * 32, expected.data() + i * 32, 32) == 0;
    return ok;
  }

  static int64_t total_units(const FileList& files, int64_t piece_len) {
    int64_t n = 0;
    for (const auto& f : files) n += mp::unit_count(f.second, piece_len);
    return n;
  }

  // Kernel-only timing on device-resident data (hipEvents): ms per sha256_leaves launch over
  // n_leaves full leaves, and the summed ms of the log2(n_leaves) sha256_pairs launches that
  // reduce them to one root. n_leaves: a power of two.
  std::vector<double> kernel_bench(int64_t n_leaves, int iters) {
    HIP_CHECK(hipSetDevice(device_));
    DevMem<uint8_t> data((size_t)(n_leaves * kLeaf)), da((size_t)n_leaves * 32),
        db((size_t)n_leaves * 32);
    DevEvent e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
    hipStream_t st = stream_[0];
    HIP_CHECK(hipMemsetAsync(data.p, 0x5a, (size_t)(n_leaves * kLeaf), st));
    double t[2] = {0, 0};
    for (int it = 0; it < iters + 1; ++it) {
      HIP_CHECK(hipEventRecord(e0.e, st));
      launch_leaves(st, data.p, n_leaves, (int)kLeaf, da.p);
      HIP_CHECK(hipEventRecord(e1.e, st));
      uint8_t *cur = da.p, *nxt = db.p;
      for (int64_t m = n_leaves; m > 1; m >>= 1, std::swap(cur, nxt))
        launch_pairs(st, cur, m / 2, nxt);
      HIP_CHECK(hipEventRecord(e2.e, st));
      HIP_CHECK(hipEventSynchronize(e2.e));
      float ms0 = 0, ms1 = 0;
      HIP_CHECK(hipEventElapsedTime(&ms0, e0.e, e1.e));
      HIP_CHECK(hipEventElapsedTime(&ms1, e1.e, e2.e));
      if (it > 0) t[0] += ms0, t[1] += ms1;
    }
    return {t[0] / iters, t[1] / iters};
  }

  static int64_t num_pieces(int64_t length, int64_t piece_len) {
    return length > piece_len ? (length + piece_len - 1) / piece_len : 1;
  }

 private:
  void release() {
    hipSetDevice(device_);
    for (int s = 0; s < 2; ++s) {
      if (stream_[s]) hipStreamSynchronize(stream_[s]);
      if (h_buf_[s]) hipHostFree(h_buf_[s]);
      if (d_buf_[s]) hipFree(d_buf_[s]);
      if (h_dig_[s]) hipHostFree(h_dig_[s]);
      for (int b = 0; b < 2; ++b)
        if (d_dig_[s][b]) hipFree(d_dig_[s][b]);
      if (h_tab_[s]) hipHostFree(h_tab_[s]);
      if (d_tab_[s]) hipFree(d_tab_[s]);
      if (d_res_[s]) hipFree(d_res_[s]);
      if (stream_[s]) hipStreamDestroy(stream_[s]);
      stream_[s] = nullptr;
      h_buf_[s] = d_buf_[s] = h_dig_[s] = d_dig_[s][0] = d_dig_[s][1] = d_res_[s] = nullptr;
      h_tab_[s] = d_tab_[s] = nullptr;
    }
  }

  // Leaf tables (pinned host + device) and the per-unit result buffers of the multi-file
  // entries: one per slot, sized for batch_bytes / 16384 leaves and units, allocated by the
  // first hash_files / verify_files call.
  void ensure_plan_buffers() {
    const size_t cap = (size_t)(batch_bytes_ / kLeaf);
    for (int s = 0; s < 2; ++s) {
      if (!h_tab_[s])
        HIP_CHECK(hipHostMalloc((void**)&h_tab_[s], cap * sizeof(PlanLeaf), hipHostMallocDefault));
      if (!d_tab_[s]) HIP_CHECK(hipMalloc((void**)&d_tab_[s], cap * sizeof(PlanLeaf)));
      if (!d_res_[s]) HIP_CHECK(hipMalloc((void**)&d_res_[s], dig_bytes_));
    }
  }

  // Reads of batch `b` into slot s: the reader threads work through the read list in ranges
  // of at most kFillChunk, each opening the file for its range and closing it again (a batch
  // may name tens of thousands of files). What pread did not deliver is zeroed. A unit its file
  // does not cover is marked 0 in `readable` (one byte per unit of the batch); without
  // `readable` it is an error.
  void fill_batch(const FileList& files, const mp::Batch& b, int s, uint8_t* readable) {
    struct Chunk {
      size_t read;
      int64_t off, len;
    };
    std::vector<Chunk> chunks;
    for (size_t r = 0; r < b.reads.size(); ++r)
      for (int64_t o = 0; o < b.reads[r].len; o += kFillChunk)
        chunks.push_back(Chunk{r, o, std::min(kFillChunk, b.reads[r].len - o)});
    std::vector<std::atomic<int64_t>> good(b.reads.size());  // delivered prefix per read
    for (size_t r = 0; r < b.reads.size(); ++r) good[r].store(b.reads[r].len);
    parallel_for(chunks.size(), readers_, [&](size_t c) {
      const Chunk& ch = chunks[c];
      const mp::Read& rd = b.reads[ch.read];
      uint8_t* dst = h_buf_[s] + rd.slot_off + ch.off;
      int64_t got = 0;
      {
        Fd f(files[(size_t)rd.file].first);
        while (f.fd >= 0 && got < ch.len) {
          ssize_t n = pread(f.fd, dst + got, (size_t)(ch.len - got), rd.file_off + ch.off + got);
          if (n < 0 && errno == EINTR) continue;
          if (n <= 0) break;
          got += n;
        }
      }
      if (got < ch.len) {
        memset(dst + got, 0, (size_t)(ch.len - got));
        int64_t at = ch.off + got, cur = good[ch.read].load();
        while (at < cur && !good[ch.read].compare_exchange_weak(cur, at)) {
        }
      }
    });
    size_t u = 0;  // units and reads are both in file order, one read per file of the batch
    for (size_t r = 0; r < b.reads.size(); ++r) {
      const mp::Read& rd = b.reads[r];
      const int64_t g = good[r].load();
      for (; u < b.units.size() && b.units[u].file == rd.file; ++u) {
        if (b.units[u].slot_off + b.units[u].bytes - rd.slot_off <= g) continue;
        if (!readable)
          throw std::runtime_error("cannot read " + files[(size_t)rd.file].first + ": short at byte " +
                                   std::to_string(rd.file_off + g));
        readable[u] = 0;
      }
    }
  }

  // The batch loop of the multi-file entries: 32 bytes per unit into `nodes`. Batch i + 1 is
  // planned and read into its slot while batch i copies and hashes on the other slot's stream;
  // a slot is drained only when it comes round again, so fills and device work overlap across
  // file boundaries. Per batch: two H2D copies (data, leaf table), one memset of the level-0
  // digests when leaves are missing, ONE sha256_leaf_table launch, one D2D copy of the width-1
  // units' leaf digests, ONE sha256_pairs_fin launch per level and one D2H copy of the nodes.
  void run_files(const FileList& files, int64_t piece_len, uint8_t* nodes, uint8_t* readable) {
    HIP_CHECK(hipSetDevice(device_));
    ensure_plan_buffers();
    std::vector<int64_t> lengths;
    lengths.reserve(files.size());
    for (const auto& f : files) lengths.push_back(f.second);
    mp::Planner planner(std::move(lengths), piece_len, batch_bytes_);
    mp::Batch plan[2];
    bool live[2] = {false, false};
    auto drain = [&](int s) {
      if (!live[s]) return;
      live[s] = false;
      HIP_CHECK(hipStreamSynchronize(stream_[s]));
      const mp::Batch& b = plan[s];
      for (size_t j = 0; j < b.order.size(); ++j)  // sorted position -> (file, piece) order
        memcpy(nodes + (b.first_unit + b.order[j]) * 32, h_dig_[s] + j * 32, 32);
    };
    try {
      for (int s = 0;; s ^= 1) {
        drain(s);  // slot s free again (its previous batch has completed)
        if (!planner.next(plan[s])) break;
        const mp::Batch& b = plan[s];
        fill_batch(files, b, s, readable ? readable + b.first_unit : nullptr);
        const int64_t nl = (int64_t)b.leaves.size(), nu = (int64_t)b.units.size();
        memcpy(h_tab_[s], b.leaves.data(), (size_t)nl * sizeof(PlanLeaf));
        hipStream_t st = stream_[s];
        HIP_CHECK(hipMemcpyAsync(d_buf_[s], h_buf_[s], (size_t)b.data_bytes,
                                 hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_tab_[s], h_tab_[s], (size_t)nl * sizeof(PlanLeaf),
                                 hipMemcpyHostToDevice, st));
        if (nl < b.width_sum)  // missing leaves: 32 zero bytes each
          HIP_CHECK(hipMemsetAsync(d_dig_[s][0], 0, (size_t)b.width_sum * 32, st));
        launch_leaf_table(st, d_buf_[s], d_tab_[s], nl, d_dig_[s][0]);
        if (b.w1_count)  // width-1 units: their leaf is their node, the tail of both orders
          HIP_CHECK(hipMemcpyAsync(d_res_[s] + (nu - b.w1_count) * 32,
                                   d_dig_[s][0] + (b.width_sum - b.w1_count) * 32,
                                   (size_t)b.w1_count * 32, hipMemcpyDeviceToDevice, st));
        int cur = 0;
        for (const mp::Level& lv : b.levels) {
          launch_pairs_fin(st, d_dig_[s][cur], lv, d_dig_[s][cur ^ 1], d_res_[s]);
          cur ^= 1;
        }
        HIP_CHECK(hipMemcpyAsync(h_dig_[s], d_res_[s], (size_t)nu * 32, hipMemcpyDeviceToHost, st));
        live[s] = true;
      }
      drain(0);
      drain(1);
    } catch (...) {
      // nothing of this call stays in flight on the slots the next call reuses
      for (int s = 0; s < 2; ++s)
        if (hipStreamSynchronize(stream_[s]) != hipSuccess) (void)hipGetLastError();
      throw;
    }
  }

  // BEP 52 tree of `length` bytes. A file no larger than a piece has no layer: its root is
  // taken over its leaves padded with zero leaves to the next power of two (not to the piece
  // size), which is the one "piece" of a tree whose piece length is that power of two.
  template <class Fill>
  Tree tree(int64_t length, int64_t piece_len, Fill&& fill, uint8_t* readable,
            bool want_root = true) {
    Tree t;
    if (length <= piece_len) {
      const int64_t eff = kLeaf * pow2_ceil((length + kLeaf - 1) / kLeaf);
      t.root.assign(32, '\0');
      run(length, eff, fill, (uint8_t*)t.root.data(), readable);
      return t;
    }
    const int64_t np = (length + piece_len - 1) / piece_len;
    t.layer.assign((size_t)np * 32, '\0');
    run(length, piece_len, fill, (uint8_t*)t.layer.data(), readable);
    if (want_root) t.root = reduce_to_root(t.layer, log2_exact(piece_len / kLeaf));
    return t;
  }

  // Root over a piece layer at tree level `level`, padded to a power of two with that level's
  // pad hash; one sha256_pairs launch per level above it.
  std::string reduce_to_root(const std::string& layer, int level) {
    const int64_t np = (int64_t)layer.size() / 32, P = pow2_ceil(np);
    const Digest pad = pad_hash(level);
    std::string in((size_t)P * 32, '\0');
    memcpy(&in[0], layer.data(), layer.size());
    for (int64_t i = np; i < P; ++i) memcpy(&in[(size_t)i * 32], pad.data(), 32);
    HIP_CHECK(hipSetDevice(device_));
    DevMem<uint8_t> da(in.size()), db(std::max<size_t>(32, in.size() / 2));
    hipStream_t st = stream_[0];
    HIP_CHECK(hipMemcpyAsync(da.p, in.data(), in.size(), hipMemcpyHostToDevice, st));
    uint8_t *cur = da.p, *nxt = db.p;
    for (int64_t m = P; m > 1; m >>= 1, std::swap(cur, nxt)) launch_pairs(st, cur, m / 2, nxt);
    std::string root(32, '\0');
    HIP_CHECK(hipMemcpyAsync(&root[0], cur, 32, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return root;
  }

  // The batch loop: 32 bytes per piece of piece_len (a power of two >= 16 KiB, <= batch_bytes)
  // into layer_out. Slot s is filled by the reader threads while the other slot's stream copies
  // and hashes; a slot's digests are collected when it comes round again. With `readable`, a
  // piece the fill could not deliver whole is marked 0 there (and hashed over zeroes);
  // without it a short fill is an error.
  template <class Fill>
  void run(int64_t length, int64_t piece_len, Fill&& fill, uint8_t* layer_out, uint8_t* readable) {
    HIP_CHECK(hipSetDevice(device_));
    const int64_t np = (length + piece_len - 1) / piece_len;
    const int64_t L = piece_len / kLeaf;
    const int levels = log2_exact(L);
    const int64_t per = batch_bytes_ / piece_len;  // >= 1: checked by the caller
    struct Pending {
      int64_t first = 0, cnt = 0;
      bool live = false;
    } pend[2];
    auto drain = [&](int s) {
      if (!pend[s].live) return;
      pend[s].live = false;
      HIP_CHECK(hipStreamSynchronize(stream_[s]));
      memcpy(layer_out + pend[s].first * 32, h_dig_[s], (size_t)pend[s].cnt * 32);
    };
    try {
      int s = 0;
      for (int64_t first = 0; first < np; first += per, s ^= 1) {
        const int64_t cnt = std::min(per, np - first);
        drain(s);  // slot s free again (its previous batch has completed)
        const int64_t off = first * piece_len;
        const int64_t bytes = std::min(cnt * piece_len, length - off);
        const int64_t good = fill(off, bytes, h_buf_[s]);
        if (good < bytes) {
          if (!readable) throw std::runtime_error("short read at byte " + std::to_string(off + good));
          memset(h_buf_[s] + good, 0, (size_t)(bytes - good));
          for (int64_t k = good / piece_len; k < cnt; ++k) readable[(size_t)(first + k)] = 0;
        }
        hipStream_t st = stream_[s];
        HIP_CHECK(hipMemcpyAsync(d_buf_[s], h_buf_[s], (size_t)bytes, hipMemcpyHostToDevice, st));
        const int64_t nl = (bytes + kLeaf - 1) / kLeaf;
        const int last_len = (int)(bytes - (nl - 1) * kLeaf);
        launch_leaves(st, d_buf_[s], nl, last_len, d_dig_[s][0]);
        int64_t m = cnt * L;
        if (nl < m)  // missing leaves of the file's last piece: 32 zero bytes each
          HIP_CHECK(hipMemsetAsync(d_dig_[s][0] + nl * 32, 0, (size_t)(m - nl) * 32, st));
        int cur = 0;
        for (int lv = 0; lv < levels; ++lv, m >>= 1, cur ^= 1)
          launch_pairs(st, d_dig_[s][cur], m / 2, d_dig_[s][cur ^ 1]);
        HIP_CHECK(hipMemcpyAsync(h_dig_[s], d_dig_[s][cur], (size_t)cnt * 32,
                                 hipMemcpyDeviceToHost, st));
        pend[s].first = first;
        pend[s].cnt = cnt;
        pend[s].live = true;
      }
      drain(0);
      drain(1);
    } catch (...) {
      // nothing of this call stays in flight on the slots the next call reuses
      for (int s = 0; s < 2; ++s)
        if (hipStreamSynchronize(stream_[s]) != hipSuccess) (void)hipGetLastError();
      throw;
    }
  }

  int device_;
  int64_t batch_bytes_;
  int readers_;
  size_t dig_bytes_ = 0;
  hipStream_t stream_[2] = {nullptr, nullptr};
  uint8_t* h_buf_[2] = {nullptr, nullptr};
  uint8_t* d_buf_[2] = {nullptr, nullptr};
  uint8_t* h_dig_[2] = {nullptr, nullptr};
  uint8_t* d_dig_[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  PlanLeaf* h_tab_[2] = {nullptr, nullptr};  // see ensure_plan_buffers
  PlanLeaf* d_tab_[2] = {nullptr, nullptr};
  uint8_t* d_res_[2] = {nullptr, nullptr};
  std::vector<Digest> pads_;
};

// The buffer entry points hash size * itemsize bytes from info.ptr, which are the view's bytes
// only when it is one C-ordered run: a stepped, reversed or column slice is refused
// (ValueError) before any HIP call. Extents of 1 may carry any stride; an empty view is
// contiguous.
void require_c_contiguous(const py::buffer_info& info) {
  if (info.size == 0) return;
  py::ssize_t want = info.itemsize;
  for (py::ssize_t d = info.ndim; d-- > 0;) {
    if (info.shape[(size_t)d] != 1 && info.strides[(size_t)d] != want)
      throw std::invalid_argument("buffer must be C-contiguous");
    want *= info.shape[(size_t)d];
  }
}

// Checked before any HIP call (std::invalid_argument -> ValueError).
void require_piece_len(const MerkleHasher& h, int64_t piece_len) {
  if (piece_len < kLeaf || !is_pow2(piece_len))
    throw std::invalid_argument("piece_len must be a power of two, at least 16384");
  if (piece_len > h.batch_bytes())
    throw std::invalid_argument("piece_len exceeds the hasher's batch_bytes");
}

void require_files(const FileList& files) {
  if (files.empty()) throw std::invalid_argument("files must not be empty");
  for (const auto& f : files)
    if (f.second <= 0) throw std::invalid_argument("length must be > 0");
}

py::tuple tree_tuple(const Tree& t) { return py::make_tuple(py::bytes(t.layer), py::bytes(t.root)); }

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

}  // namespace

PYBIND11_MODULE(_gpumerkle, m) {
  m.doc() = "gfx950 BEP 52 merkle hashing (SHA-256: one lane per 16 KiB block, one per parent)";
  m.def("device_count", &device_count);
  m.def("arch", [] {
    hipDeviceProp_t p;
    HIP_CHECK(hipGetDeviceProperties(&p, 0));
    return std::string(p.gcnArchName);
  });
  py::class_<MerkleHasher>(m, "MerkleHasher")
      .def(py::init([](int device, int64_t batch_bytes, int readers) {
             if (batch_bytes < kLeaf)
               throw std::invalid_argument("batch_bytes must be at least 16384");
             py::gil_scoped_release rel;
             return new MerkleHasher(device, batch_bytes, readers);
           }),
           py::arg("device") = 0, py::arg("batch_bytes") = (int64_t)256 << 20,
           py::arg("reader_threads") = 8)
      .def(
          "leaf_hashes",
          [](MerkleHasher& h, const py::buffer& b) {
            py::buffer_info info = b.request();
            require_c_contiguous(info);
            const int64_t n = (int64_t)info.size * (int64_t)info.itemsize;
            std::string out;
            {
              py::gil_scoped_release rel;
              out = h.leaf_hashes((const uint8_t*)info.ptr, n);
            }
            return py::bytes(out);
          },
          py::arg("data"), "32 bytes per 16 KiB block of a C-contiguous buffer")
      .def(
          "reduce_layer",
          [](MerkleHasher& h, const py::bytes& hashes, const py::bytes& pad) {
            std::string hs = hashes, pd = pad;
            if (hs.empty() || hs.size() % 32)
              throw std::invalid_argument("hashes must be k x 32 bytes, k >= 1");
            if (pd.size() != 32) throw std::invalid_argument("pad must be 32 bytes");
            std::string out;
            {
              py::gil_scoped_release rel;
              out = h.reduce_layer(hs, pd);
            }
            return py::bytes(out);
          },
          py::arg("hashes"), py::arg("pad"),
          "One tree level: ceil(k / 2) x 32 bytes; an odd k is completed with `pad`")
      .def(
          "pad_hash",
          [](MerkleHasher& h, int level) {
            Digest d;
            {
              py::gil_scoped_release rel;
              d = h.pad_hash(level);
            }
            return py::bytes((const char*)d.data(), d.size());
          },
          py::arg("level"), "Hash of an all-missing subtree of 2**level leaves")
      .def(
          "hash_buffer",
          [](MerkleHasher& h, const py::buffer& b, int64_t piece_len) {
            py::buffer_info info = b.request();
            require_c_contiguous(info);
            require_piece_len(h, piece_len);
            const int64_t n = (int64_t)info.size * (int64_t)info.itemsize;
            if (n == 0) throw std::invalid_argument("an empty file has no merkle tree");
            Tree t;
            {
              py::gil_scoped_release rel;
              t = h.hash_buffer((const uint8_t*)info.ptr, n, piece_len);
            }
            return tree_tuple(t);
          },
          py::arg("data"), py::arg("piece_len"), "(piece_layer, root) of one file held in memory")
      .def(
          "hash_file",
          [](MerkleHasher& h, const std::string& path, int64_t length, int64_t piece_len) {
            require_piece_len(h, piece_len);
            if (length <= 0) throw std::invalid_argument("length must be > 0");
            Tree t;
            {
              py::gil_scoped_release rel;
              t = h.hash_file(path, length, piece_len);
            }
            return tree_tuple(t);
          },
          py::arg("path"), py::arg("length"), py::arg("piece_len"),
          "(piece_layer, root) of the first `length` bytes of a file, streamed in batches")
      .def(
          "verify_file",
          [](MerkleHasher& h, const std::string& path, int64_t length, int64_t piece_len,
             const py::bytes& expected) {
            require_piece_len(h, piece_len);
            if (length <= 0) throw std::invalid_argument("length must be > 0");
            std::string ex = expected;
            if ((int64_t)ex.size() != MerkleHasher::num_pieces(length, piece_len) * 32)
              throw std::invalid_argument(
                  "expected must be the piece layer (32 bytes per piece), or the 32-byte root of "
                  "a file no larger than a piece");
            std::vector<uint8_t> ok;
            {
              py::gil_scoped_release rel;
              ok = h.verify_file(path, length, piece_len, ex);
            }
            return py::bytes((const char*)ok.data(), ok.size());
          },
          py::arg("path"), py::arg("length"), py::arg("piece_len"), py::arg("expected"),
          "One byte per piece (1 = good) against the piece layer, or against the pieces root for "
          "a file no larger than a piece; pieces a missing or short file cannot cover are 0")
      .def(
          "hash_files",
          [](MerkleHasher& h, const FileList& files, int64_t piece_len) {
            require_piece_len(h, piece_len);
            require_files(files);
            std::string out;
            {
              py::gil_scoped_release rel;
              out = h.hash_files(files, piece_len);
            }
            return py::bytes(out);
          },
          py::arg("files"), py::arg("piece_len"),
          "32 bytes per unit of `files` [(path, length)], file order then piece order: the piece "
          "layer of a file longer than a piece, the pieces root of a smaller one. Pieces of many "
          "files share a device batch")
      .def(
          "verify_files",
          [](MerkleHasher& h, const FileList& files, int64_t piece_len, const py::bytes& expected) {
            require_piece_len(h, piece_len);
            require_files(files);
            std::string ex = expected;
            if ((int64_t)ex.size() != MerkleHasher::total_units(files, piece_len) * 32)
              throw std::invalid_argument(
                  "expected must hold, per file in order, the piece layer or the 32-byte root of "
                  "a file no larger than a piece");
            std::vector<uint8_t> ok;
            {
              py::gil_scoped_release rel;
              ok = h.verify_files(files, piece_len, ex);
            }
            return py::bytes((const char*)ok.data(), ok.size());
          },
          py::arg("files"), py::arg("piece_len"), py::arg("expected"),
          "One byte per unit (1 = good) in the order of hash_files; units a missing or short file "
          "cannot cover are 0")
      .def(
          "kernel_bench",
          [](MerkleHasher& h, int64_t n_leaves, int iters) {
            if (n_leaves < 2 || !is_pow2(n_leaves) || iters <= 0)
              throw std::invalid_argument("n_leaves must be a power of two >= 2, iters > 0");
            std::vector<double> r;
            {
              py::gil_scoped_release rel;
              r = h.kernel_bench(n_leaves, iters);
            }
            return py::make_tuple(r[0], r[1]);
          },
          py::arg("n_leaves"), py::arg("iters") = 3,
          "(ms per sha256_leaves launch, summed ms of the sha256_pairs launches that reduce the "
          "leaves to one root): device-resident data")
      .def_property_readonly("batch_bytes", &MerkleHasher::batch_bytes);
}
