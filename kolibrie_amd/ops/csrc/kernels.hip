// kolibrie_amd native CDNA4 kernels (gfx950 / MI355X).
//
// MI355X-native implementations of the engine's hot loops:
//   K1 scan_probe  — per-binding-row index probe: binary-search range over a
//                    sorted packed-key permutation, two-pass count+emit.
//                    (replaces reference engine.rs:1018-1251 scan loops)
//   K2 hash_join   — chained open-addressing hash join over k int32 key
//                    columns, build+count+emit.
//                    (replaces engine.rs:1367 hash_join_solution_sequences
//                     and shared/src/join_algorithm.rs:64-265)
//   K5 filter      — postfix-bytecode predicate over id columns + the f64
//                    value column (replaces types.rs:373 evaluate_with_ids).
//   K9 str_match   — STRSTARTS / STRENDS / CONTAINS / literal REGEX over the
//                    device term-text table (the reference evaluates these
//                    to false).
//   K11 term_order — ORDER BY collation: per-round sort keys, common-prefix
//                    skip and numeric classification over the term-text
//                    table (replaces the per-row decode + sorted() of
//                    execute_query.rs:477's port).
//   K12 path_reach — property paths from a bound endpoint: multi-source
//                    level-synchronous BFS over a CSR adjacency, 64 sources
//                    per pass as the bits of per-node uint64 masks.
//   K14 left_join  — OPTIONAL as LeftJoin(A, P, F): the K2 table over the
//                    right side, the K5 program run on every key-equal pair
//                    inside the chain walk, count + emit + matched flags.
//
// Design notes (per CDNA4 guide): wave64, 256-thread blocks, grid-stride
// loops capped so the 256-CU chip is saturated without oversubscription;
// all data int32/int64 columns in HBM — memory-latency-bound probes rely on
// high occupancy; atomics are agent-scope (device) by default.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string_view>
#include <cstring>
#include <thread>
#include <unordered_map>

namespace py = pybind11;
#include <vector>

#define HIP_OK(expr)                                                          \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));      \
  } while (0)

namespace {

constexpr int kBlock = 256;

inline int grid_for(int64_t n) {
  int64_t blocks = (n + kBlock - 1) / kBlock;
  // 256 CUs x 8 blocks/CU: cap and grid-stride the rest (guide G11)
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks);
}

__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* __restrict__ a,
                                                   int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t upper_bound_i64(const int64_t* __restrict__ a,
                                                   int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- K1: probe
// Row i of a probe asks for the index rows whose packed key lies in
// [lo(i), hi(i)].  The three key shapes differ only in how that pair is
// formed; the count, tile-bounds and emit kernels are shared.

// exact mode: probe key = packed (a,b) per row
struct ExactKey {
  const int64_t* keys;
  __device__ __forceinline__ int64_t lo(int64_t i) const { return keys[i]; }
  __device__ __forceinline__ int64_t hi(int64_t i) const { return keys[i]; }
};

// range mode: the full range of leading component a (keys built from the
// int32 value)
struct RangeKey {
  const int32_t* vals;
  __device__ __forceinline__ int64_t lo(int64_t i) const {
    return static_cast<int64_t>(vals[i]) << 32;            // (v, 0x00000000)
  }
  __device__ __forceinline__ int64_t hi(int64_t i) const {
    return (static_cast<int64_t>(vals[i]) << 32) | 0xFFFFFFFFLL;  // (v, ~0)
  }
};

// fused mode: key (a<<32)|b packed inside the kernel, a/b each a per-row
// column or a broadcast constant — the engine's bind-join step then needs
// no separate pack2 pass
struct FusedKey {
  const int32_t* a_col;
  int64_t a_const;
  const int32_t* b_col;
  int64_t b_const;
  __device__ __forceinline__ int64_t lo(int64_t i) const {
    int64_t a = a_col ? static_cast<int64_t>(a_col[i]) : a_const;
    int64_t b = b_col ? static_cast<int64_t>(b_col[i]) : b_const;
    return (a << 32) | (b & 0xFFFFFFFFLL);
  }
  __device__ __forceinline__ int64_t hi(int64_t i) const { return lo(i); }
};

// ---- merge-path variant for SORTED probes ---------------------------------
// When the probe keys are themselves sorted (PSO-slice star/merge chains),
// a fully-parallel boundary pass computes each kTile-probe tile's index
// window; the count pass then searches only inside its tile window, which
// is small and cache-hot — the probe becomes a merge join.
constexpr int kTile = 768;
// fewer probes than this always take the unwindowed count
constexpr int64_t kProbeSortedMin = 262144;

template <class Key>
__global__ void probe_tile_bounds(const int64_t* __restrict__ key12, int64_t n,
                                  Key key, int64_t m, int64_t n_tiles,
                                  int64_t* __restrict__ win_lo,
                                  int64_t* __restrict__ win_hi) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tiles;
       t += (int64_t)gridDim.x * blockDim.x) {
    int64_t first = key.lo(t * kTile);
    int64_t last = key.hi(min((t + 1) * kTile - 1, m - 1));
    win_lo[t] = lower_bound_i64(key12, n, first);
    win_hi[t] = upper_bound_i64(key12, n, last);
  }
}

// count: each probe row finds its [lo, lo+cnt) index range; kWindowed
// confines the search to the row's tile window (win_lo/win_hi unused
// otherwise)
template <class Key, bool kWindowed>
__global__ void probe_count(const int64_t* __restrict__ key12, int64_t n,
                            Key key, int64_t m,
                            const int64_t* __restrict__ win_lo,
                            const int64_t* __restrict__ win_hi,
                            int64_t* __restrict__ lo_out,
                            int32_t* __restrict__ cnt_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t wlo = 0, wspan = n;
    if (kWindowed) {
      int64_t t = i / kTile;
      wlo = win_lo[t];
      wspan = win_hi[t] - wlo;
    }
    int64_t klo = key.lo(i);
    int64_t khi = key.hi(i);
    int64_t lo = wlo + lower_bound_i64(key12 + wlo, wspan, klo);
    int64_t hi = wlo + upper_bound_i64(key12 + wlo, wspan, khi);
    lo_out[i] = lo;
    cnt_out[i] = static_cast<int32_t>(hi - lo);
  }
}

// up to 4 "carry" columns are gathered by probe-row index during the emit
// pass, so the engine needs no separate gathers; k == 0 carries nothing
constexpr int kMaxCarry = 4;

struct CarryCols {
  const int32_t* in[kMaxCarry];
  int32_t* out[kMaxCarry];
  int k;
};

// emit: each probe row copies its [lo, lo+cnt) range; writes probe-row index,
// the second packed component (b, when emit_b) and the trailing column (z).
__global__ void probe_emit(const int64_t* __restrict__ key12,
                           const int32_t* __restrict__ z, int64_t m,
                           const int64_t* __restrict__ lo,
                           const int32_t* __restrict__ cnt,
                           const int64_t* __restrict__ offs,
                           CarryCols carry,
                           int64_t* __restrict__ li_out,
                           int32_t* __restrict__ b_out,
                           int32_t* __restrict__ z_out,
                           bool emit_b) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t base = offs[i];
    int64_t l = lo[i];
    int32_t c = cnt[i];
    int32_t cv[kMaxCarry];
    for (int j = 0; j < carry.k; ++j) cv[j] = carry.in[j][i];
    for (int32_t q = 0; q < c; ++q) {
      li_out[base + q] = i;
      if (emit_b)
        b_out[base + q] = static_cast<int32_t>(key12[l + q] & 0xFFFFFFFFLL);
      z_out[base + q] = z[l + q];
      for (int j = 0; j < carry.k; ++j) carry.out[j][base + q] = cv[j];
    }
  }
}

// balanced emit: parallel over OUTPUT elements (skew-proof — a probe row
// with 10^4 matches no longer serializes one thread); each output finds its
// probe row by binary search over the offset array.
__global__ void probe_emit_balanced(const int64_t* __restrict__ key12,
                                    const int32_t* __restrict__ z, int64_t m,
                                    const int64_t* __restrict__ lo,
                                    const int64_t* __restrict__ offs,  // [m+1]
                                    int64_t total, CarryCols carry,
                                    int64_t* __restrict__ li_out,
                                    int32_t* __restrict__ b_out,
                                    int32_t* __restrict__ z_out,
                                    bool emit_b) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    // find probe row a with offs[a] <= idx < offs[a+1]
    int64_t a = 0, b = m;
    while (a + 1 < b) {
      int64_t mid = (a + b) >> 1;
      if (offs[mid] <= idx) a = mid; else b = mid;
    }
    int64_t j = idx - offs[a];
    int64_t src = lo[a] + j;
    li_out[idx] = a;
    if (emit_b)
      b_out[idx] = static_cast<int32_t>(key12[src] & 0xFFFFFFFFLL);
    z_out[idx] = z[src];
    for (int c = 0; c < carry.k; ++c) carry.out[c][idx] = carry.in[c][a];
  }
}

// ------------------------------------------------------------- K2: hash join
constexpr int kMaxKeyCols = 4;

struct KeyCols {
  const int32_t* c[kMaxKeyCols];
  int k;
};

__device__ __forceinline__ uint64_t mix_hash(const KeyCols& kc, int64_t row) {
  // splitmix-style combine over up to 4 int32 keys
  uint64_t h = 0x9E3779B97F4A7C15ULL;
  for (int j = 0; j < kc.k; ++j) {
    uint64_t x = static_cast<uint32_t>(kc.c[j][row]);
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    h = (h ^ x) * 0x94D049BB133111EBULL;
  }
  return h ^ (h >> 31);
}

__device__ __forceinline__ bool keys_equal(const KeyCols& a, int64_t ra,
                                           const KeyCols& b, int64_t rb) {
  for (int j = 0; j < a.k; ++j)
    if (a.c[j][ra] != b.c[j][rb]) return false;
  return true;
}

__global__ void hj_build(KeyCols build, int64_t r, uint32_t mask,
                         int32_t* __restrict__ heads,
                         int32_t* __restrict__ next) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(build, i)) & mask;
    // chain push: device-scope atomic (cross-XCD safe, guide G12)
    next[i] = atomicExch(&heads[h], static_cast<int32_t>(i));
  }
}

// ---- LDS-staged variant for SMALL build sides -----------------------------
// Build sides up to 8192 rows fit a per-block chained table entirely in LDS
// (32 KB heads + 32 KB next = 64 KB -> 2 blocks/CU, 8 waves).  Every block
// rebuilds the table from the global build columns (<= 8192 LDS atomics,
// amortized over its share of probes) and the probe chain walk then costs
// LDS latency instead of L2 round trips.  This is the selective-query /
// broadcast-join shape: tiny build side, large probe side.
constexpr int kHjLdsSlots = 8192;   // heads, power of 2
constexpr int kHjLdsRows = 8192;    // max build rows

__device__ __forceinline__ void hj_lds_build(KeyCols build, int64_t r,
                                             int32_t* heads, int32_t* next) {
  for (int j = threadIdx.x; j < kHjLdsSlots; j += blockDim.x) heads[j] = -1;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < r; i += blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(build, i)) & (kHjLdsSlots - 1);
    next[i] = atomicExch(&heads[h], static_cast<int32_t>(i));
  }
  __syncthreads();
}

// The chain walks of the count and emit passes, over a table in either
// memory; forced inline so that each caller's address space is known.
__device__ __forceinline__ void hj_count_rows(
    const KeyCols& probe, int64_t l, const KeyCols& build,
    const int32_t* heads, const int32_t* next, uint32_t mask,
    int32_t* __restrict__ cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(probe, i)) & mask;
    int32_t c = 0;
    for (int32_t b = heads[h]; b >= 0; b = next[b])
      if (keys_equal(probe, i, build, b)) ++c;
    cnt[i] = c;
  }
}

__device__ __forceinline__ void hj_emit_rows(
    const KeyCols& probe, int64_t l, const KeyCols& build,
    const int32_t* heads, const int32_t* next, uint32_t mask,
    const int64_t* __restrict__ offs, int64_t* __restrict__ li_out,
    int64_t* __restrict__ ri_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(probe, i)) & mask;
    int64_t base = offs[i];
    for (int32_t b = heads[h]; b >= 0; b = next[b]) {
      if (keys_equal(probe, i, build, b)) {
        li_out[base] = i;
        ri_out[base] = b;
        ++base;
      }
    }
  }
}

// kLds: every block stages the table in LDS and ignores heads/next/mask;
// otherwise they are the global table that hj_build filled.
template <bool kLds>
__global__ void hj_count(KeyCols probe, int64_t l, KeyCols build, int64_t r,
                         const int32_t* __restrict__ heads,
                         const int32_t* __restrict__ next, uint32_t mask,
                         int32_t* __restrict__ cnt) {
  if constexpr (kLds) {
    __shared__ int32_t lds_heads[kHjLdsSlots];
    __shared__ int32_t lds_next[kHjLdsRows];
    hj_lds_build(build, r, lds_heads, lds_next);
    hj_count_rows(probe, l, build, lds_heads, lds_next, kHjLdsSlots - 1, cnt);
  } else {
    hj_count_rows(probe, l, build, heads, next, mask, cnt);
  }
}

template <bool kLds>
__global__ void hj_emit(KeyCols probe, int64_t l, KeyCols build, int64_t r,
                        const int32_t* __restrict__ heads,
                        const int32_t* __restrict__ next, uint32_t mask,
                        const int64_t* __restrict__ offs,
                        int64_t* __restrict__ li_out,
                        int64_t* __restrict__ ri_out) {
  if constexpr (kLds) {
    __shared__ int32_t lds_heads[kHjLdsSlots];
    __shared__ int32_t lds_next[kHjLdsRows];
    hj_lds_build(build, r, lds_heads, lds_next);
    hj_emit_rows(probe, l, build, lds_heads, lds_next, kHjLdsSlots - 1, offs,
                 li_out, ri_out);
  } else {
    hj_emit_rows(probe, l, build, heads, next, mask, offs, li_out, ri_out);
  }
}

// ------------------------------------------------------------ K13: semi join
// Does probe row i have ANY build row with an equal key?  One byte per probe
// row, flipped by `anti` (NOT EXISTS).  No sort, no match counts, no emit.
//
// One or two key columns pack into one 64-bit key, and the build side becomes
// an open-addressing key SET: duplicates of a build key (the normal case, a
// pattern projected to its subject) collapse into one slot.  The halves are
// masked, not sign-extended: quoted-triple ids are negative int32.  kSemiEmpty
// is no real key: a bound two-column key would need both halves -1 (UNBOUND),
// and a one-column key has a zero low half.
//
// Three or four key columns reuse the K2 chained table; hj_exists leaves the
// chain at the first match.
constexpr unsigned long long kSemiEmpty = ~0ull;
constexpr int kSemiLdsSlots = 8192;   // 64 KB of keys: the LDS tier's limit
constexpr int kSemiMinSlots = 256;    // table floor (a power of two)
// The LDS tier copies the whole finished table into every block.  Measured
// (profiles/exists_measurements.md, section 3) it never repaid the copy: with
// 489 and 4883 probe rows per block and tables of 256, 2048 and 8192 slots it
// took as long as the table in global memory or up to 1.3x longer, so no
// amortisation bound selects it; only `lds_tier` = 1 does.

__device__ __forceinline__ unsigned long long semi_key(const KeyCols& kc,
                                                       int64_t row) {
  unsigned long long a = static_cast<uint32_t>(kc.c[0][row]);
  unsigned long long b = kc.k > 1 ? static_cast<uint32_t>(kc.c[1][row]) : 0u;
  return (a << 32) | b;
}

__device__ __forceinline__ uint32_t semi_hash(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  return static_cast<uint32_t>(x ^ (x >> 31));
}

// The table has >= 2r slots, so the load stays <= 0.5 and every walk ends.
__global__ void semi_set_build(KeyCols build, int64_t r, uint32_t mask,
                               unsigned long long* __restrict__ table) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < r;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long key = semi_key(build, i);
    uint32_t h = semi_hash(key) & mask;
    for (;;) {
      // a slot only ever goes EMPTY -> key, so a plain load that already
      // shows the key spares the atomic (duplicate build keys)
      unsigned long long cur = table[h];
      if (cur == key) break;
      if (cur == kSemiEmpty) {
        // device-scope atomic (cross-XCD safe, guide G12)
        cur = atomicCAS(&table[h], kSemiEmpty, key);
        if (cur == kSemiEmpty || cur == key) break;
      }
      h = (h + 1) & mask;
    }
  }
}

__device__ __forceinline__ void semi_probe_rows(
    const KeyCols& probe, int64_t l, const unsigned long long* table,
    uint32_t mask, uint8_t anti, uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long key = semi_key(probe, i);
    uint32_t h = semi_hash(key) & mask;
    uint8_t found = 0;
    for (;;) {
      unsigned long long cur = table[h];
      if (cur == key) { found = 1; break; }
      if (cur == kSemiEmpty) break;
      h = (h + 1) & mask;
    }
    out[i] = found ^ anti;
  }
}

// kLds: the finished table (mask + 1 <= kSemiLdsSlots slots) is copied into
// LDS with 16-byte loads, a plain copy and not a rebuild, then probed there.
template <bool kLds>
__global__ void semi_set_probe(KeyCols probe, int64_t l,
                               const unsigned long long* __restrict__ table,
                               uint32_t mask, uint8_t anti,
                               uint8_t* __restrict__ out) {
  if constexpr (kLds) {
    __shared__ __attribute__((aligned(16)))
        unsigned long long lds_table[kSemiLdsSlots];
    const uint4* src = reinterpret_cast<const uint4*>(table);
    uint4* dst = reinterpret_cast<uint4*>(lds_table);
    const int n16 = static_cast<int>((mask + 1u) >> 1);   // two slots a load
    for (int j = threadIdx.x; j < n16; j += blockDim.x) dst[j] = src[j];
    __syncthreads();
    semi_probe_rows(probe, l, lds_table, mask, anti, out);
  } else {
    semi_probe_rows(probe, l, table, mask, anti, out);
  }
}

__device__ __forceinline__ void hj_exists_rows(
    const KeyCols& probe, int64_t l, const KeyCols& build,
    const int32_t* heads, const int32_t* next, uint32_t mask, uint8_t anti,
    uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(probe, i)) & mask;
    uint8_t found = 0;
    for (int32_t b = heads[h]; b >= 0; b = next[b])
      if (keys_equal(probe, i, build, b)) { found = 1; break; }
    out[i] = found ^ anti;
  }
}

// hj_count without the count: the chain walk leaves at the first match.
template <bool kLds>
__global__ void hj_exists(KeyCols probe, int64_t l, KeyCols build, int64_t r,
                          const int32_t* __restrict__ heads,
                          const int32_t* __restrict__ next, uint32_t mask,
                          uint8_t anti, uint8_t* __restrict__ out) {
  if constexpr (kLds) {
    __shared__ int32_t lds_heads[kHjLdsSlots];
    __shared__ int32_t lds_next[kHjLdsRows];
    // the staging of hj_lds_build, on the kernel argument itself: a copy of
    // KeyCols indexed in a loop would live in scratch
    for (int j = threadIdx.x; j < kHjLdsSlots; j += blockDim.x)
      lds_heads[j] = -1;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < r; i += blockDim.x) {
      uint32_t h =
          static_cast<uint32_t>(mix_hash(build, i)) & (kHjLdsSlots - 1);
      lds_next[i] = atomicExch(&lds_heads[h], static_cast<int32_t>(i));
    }
    __syncthreads();
    hj_exists_rows(probe, l, build, lds_heads, lds_next, kHjLdsSlots - 1, anti,
                   out);
  } else {
    hj_exists_rows(probe, l, build, heads, next, mask, anti, out);
  }
}

// ------------------------------------------------------------ K5: filter VM
// Postfix bytecode over binding columns.  Opcodes (engine/filter_bytecode.py
// must match):
enum FilterOp : int32_t {
  OP_PUSH_ID = 0,     // arg: column index      -> id stack
  OP_PUSH_CONST_ID,   // arg: literal id        -> id stack
  OP_PUSH_VAL,        // arg: column index      -> val stack (value_col[id])
  OP_PUSH_CONST_VAL,  // arg: f64 const index   -> val stack
  OP_EQ_ID,           // id x id -> bool
  OP_NE_ID,
  OP_LT, OP_GT, OP_LE, OP_GE,    // val x val -> bool
  OP_EQ_VAL, OP_NE_VAL,
  OP_ADD, OP_SUB, OP_MUL, OP_DIV,  // val x val -> val
  OP_AND, OP_OR, OP_NOT,           // bool
  OP_BOUND,           // arg: column index -> bool (id != UNBOUND)
  OP_IS_TRIPLE,       // id -> bool
  OP_PUSH_TRUE, OP_PUSH_FALSE,
};

constexpr int kMaxStack = 16;
constexpr int kMaxCols = 16;
constexpr int32_t kUnbound = -1;

struct FilterProg {
  const int32_t* ops;      // [n_ops]
  const int32_t* args;     // [n_ops]
  const double* consts;    // f64 constant pool
  int n_ops;
};

struct BindCols {
  const int32_t* c[kMaxCols];
  int k;
  // cell of column slot a for the row under test (K5 has one row index)
  __device__ __forceinline__ int32_t at(int32_t a, int64_t row, int64_t) const {
    return c[a][row];
  }
};

// One evaluation of the program.  `cols.at(a, i, b)` reads the cell of column
// slot a for the row i (K5) or the pair of rows (i, b) (K14) under test.
// Forced inline and handed the kernel's column argument by reference, so each
// kernel indexes that argument in place (a closure over it lands in scratch).
template <typename Cols>
__device__ __forceinline__ bool filter_vm(const FilterProg& prog,
                                          const double* __restrict__ value_col,
                                          int64_t value_n, const Cols& cols,
                                          int64_t i, int64_t b) {
  int32_t ids[kMaxStack];
  double vals[kMaxStack];
  // the boolean stack and the validity (NaN / div0) of each val slot are
  // bit stacks: bit s is slot s
  uint32_t bools = 0, ok = 0;
  int si = 0, sv = 0, sb = 0;
  auto push_b = [&](bool r) {
    bools = (bools & ~(1u << sb)) | (static_cast<uint32_t>(r) << sb);
    ++sb;
  };
  auto set_ok = [&](int s, bool v) {
    ok = (ok & ~(1u << s)) | (static_cast<uint32_t>(v) << s);
  };
  for (int pc = 0; pc < prog.n_ops; ++pc) {
    int32_t op = prog.ops[pc];
    int32_t a = prog.args[pc];
    switch (op) {
      case OP_PUSH_ID: ids[si++] = cols.at(a, i, b); break;
      case OP_PUSH_CONST_ID: ids[si++] = a; break;
      case OP_PUSH_VAL: {
        int32_t id = cols.at(a, i, b);
        int64_t u = static_cast<uint32_t>(id);
        double v = (u < value_n && id != kUnbound) ? value_col[u] : 0.0;
        vals[sv] = v; set_ok(sv, id != kUnbound); ++sv;
        break;
      }
      case OP_PUSH_CONST_VAL: vals[sv] = prog.consts[a]; set_ok(sv, true); ++sv; break;
      case OP_EQ_ID: { bool r = ids[si-2] == ids[si-1] && ids[si-2] != kUnbound;
                       si -= 2; push_b(r); break; }
      case OP_NE_ID: { bool r = ids[si-2] != ids[si-1] && ids[si-2] != kUnbound
                                && ids[si-1] != kUnbound;
                       si -= 2; push_b(r); break; }
      case OP_LT: case OP_GT: case OP_LE: case OP_GE:
      case OP_EQ_VAL: case OP_NE_VAL: {
        double x = vals[sv-2], y = vals[sv-1];
        bool v = ((ok >> (sv-2)) & 3u) == 3u;
        sv -= 2;
        bool r = false;
        if (op == OP_LT) r = x < y;
        else if (op == OP_GT) r = x > y;
        else if (op == OP_LE) r = x <= y;
        else if (op == OP_GE) r = x >= y;
        else if (op == OP_EQ_VAL) r = x == y;
        else r = x != y;
        push_b(r && v);
        break;
      }
      case OP_ADD: case OP_SUB: case OP_MUL: case OP_DIV: {
        double x = vals[sv-2], y = vals[sv-1];
        bool v = ((ok >> (sv-2)) & 3u) == 3u;
        sv -= 2;
        double r = 0.0;
        if (op == OP_ADD) r = x + y;
        else if (op == OP_SUB) r = x - y;
        else if (op == OP_MUL) r = x * y;
        else { if (y == 0.0) v = false; else r = x / y; }
        vals[sv] = r; set_ok(sv, v); ++sv;
        break;
      }
      case OP_AND: { bool r = ((bools >> (sb-2)) & 3u) == 3u; sb -= 2; push_b(r); break; }
      case OP_OR:  { bool r = ((bools >> (sb-2)) & 3u) != 0u; sb -= 2; push_b(r); break; }
      case OP_NOT: bools ^= 1u << (sb-1); break;
      case OP_BOUND: push_b(cols.at(a, i, b) != kUnbound); break;
      case OP_IS_TRIPLE: { int32_t id = ids[--si];
                           push_b((id < 0) && (id != kUnbound)); break; }
      case OP_PUSH_TRUE: push_b(true); break;
      case OP_PUSH_FALSE: push_b(false); break;
    }
  }
  return sb > 0 ? ((bools >> (sb-1)) & 1u) != 0u : false;
}

__global__ void filter_eval(FilterProg prog, BindCols cols,
                            const double* __restrict__ value_col,
                            int64_t value_n, int64_t n,
                            bool* __restrict__ out) {
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    out[row] = filter_vm(prog, value_col, value_n, cols, row, row);
  }
}

// ----------------------------------------------------------- K14: left join
// OPTIONAL as LeftJoin(left, right, condition): probe row i keeps the build
// rows b with an equal key on which the K5 program holds for the PAIR (i, b),
// and a probe row that keeps none is reported unmatched (the caller pads it).
// The join and the condition are one walk, since padding depends on whether
// any pair survives: a join followed by a filter has lost the rows to pad.
// Column slot a of the program is indexed by the probe row, or by the build
// row where bit a of `right_mask` is set.  An empty program passes every pair.
struct PairCols {
  const int32_t* c[kMaxCols];
  uint32_t right_mask;
  __device__ __forceinline__ int32_t at(int32_t a, int64_t i, int64_t b) const {
    return c[a][(right_mask >> a) & 1u ? b : i];
  }
};

// Count pass: survivors per probe row, and (matched != nullptr) the flag.
__device__ __forceinline__ void lj_count_rows(
    const KeyCols& probe, int64_t l, const KeyCols& build,
    const int32_t* heads, const int32_t* next, uint32_t mask,
    const FilterProg& prog, const PairCols& cols,
    const double* __restrict__ value_col, int64_t value_n,
    int32_t* __restrict__ cnt, uint8_t* __restrict__ matched) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(probe, i)) & mask;
    int32_t c = 0;
    for (int32_t b = heads[h]; b >= 0; b = next[b]) {
      if (!keys_equal(probe, i, build, b)) continue;
      if (prog.n_ops == 0 || filter_vm(prog, value_col, value_n, cols, i, b))
        ++c;
    }
    cnt[i] = c;
    if (matched != nullptr) matched[i] = c > 0;
  }
}

// Emit pass: the same walk; row i's survivors land at its exclusive offset,
// so the pairs come out grouped by ascending probe row.
__device__ __forceinline__ void lj_emit_rows(
    const KeyCols& probe, int64_t l, const KeyCols& build,
    const int32_t* heads, const int32_t* next, uint32_t mask,
    const FilterProg& prog, const PairCols& cols,
    const double* __restrict__ value_col, int64_t value_n,
    const int64_t* __restrict__ offs, int64_t* __restrict__ li_out,
    int64_t* __restrict__ ri_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(probe, i)) & mask;
    int64_t base = offs[i];
    for (int32_t b = heads[h]; b >= 0; b = next[b]) {
      if (!keys_equal(probe, i, build, b)) continue;
      if (prog.n_ops == 0 ||
          filter_vm(prog, value_col, value_n, cols, i, b)) {
        li_out[base] = i;
        ri_out[base] = b;
        ++base;
      }
    }
  }
}

// hj_lds_build on the kernel argument itself: that one takes KeyCols by value,
// and the copy, indexed in a loop, lives in scratch.
__device__ __forceinline__ void lj_lds_build(const KeyCols& build, int64_t r,
                                             int32_t* heads, int32_t* next) {
  for (int j = threadIdx.x; j < kHjLdsSlots; j += blockDim.x) heads[j] = -1;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < r; i += blockDim.x) {
    uint32_t h = static_cast<uint32_t>(mix_hash(build, i)) & (kHjLdsSlots - 1);
    next[i] = atomicExch(&heads[h], static_cast<int32_t>(i));
  }
  __syncthreads();
}

// kLds as in hj_count / hj_emit: the table over the build (right) side is
// staged per block in LDS, or it is the global one that hj_build filled.
template <bool kLds>
__global__ void lj_count(KeyCols probe, int64_t l, KeyCols build, int64_t r,
                         const int32_t* __restrict__ heads,
                         const int32_t* __restrict__ next, uint32_t mask,
                         FilterProg prog, PairCols cols,
                         const double* __restrict__ value_col,
                         int64_t value_n, int32_t* __restrict__ cnt,
                         uint8_t* __restrict__ matched) {
  if constexpr (kLds) {
    __shared__ int32_t lds_heads[kHjLdsSlots];
    __shared__ int32_t lds_next[kHjLdsRows];
    lj_lds_build(build, r, lds_heads, lds_next);
    lj_count_rows(probe, l, build, lds_heads, lds_next, kHjLdsSlots - 1, prog,
                  cols, value_col, value_n, cnt, matched);
  } else {
    lj_count_rows(probe, l, build, heads, next, mask, prog, cols, value_col,
                  value_n, cnt, matched);
  }
}

template <bool kLds>
__global__ void lj_emit(KeyCols probe, int64_t l, KeyCols build, int64_t r,
                        const int32_t* __restrict__ heads,
                        const int32_t* __restrict__ next, uint32_t mask,
                        FilterProg prog, PairCols cols,
                        const double* __restrict__ value_col, int64_t value_n,
                        const int64_t* __restrict__ offs,
                        int64_t* __restrict__ li_out,
                        int64_t* __restrict__ ri_out) {
  if constexpr (kLds) {
    __shared__ int32_t lds_heads[kHjLdsSlots];
    __shared__ int32_t lds_next[kHjLdsRows];
    lj_lds_build(build, r, lds_heads, lds_next);
    lj_emit_rows(probe, l, build, lds_heads, lds_next, kHjLdsSlots - 1, prog,
                 cols, value_col, value_n, offs, li_out, ri_out);
  } else {
    lj_emit_rows(probe, l, build, heads, next, mask, prog, cols, value_col,
                 value_n, offs, li_out, ri_out);
  }
}

// ------------------------------------------------------- K9 str_match kernels
// FILTER string predicates over the device term-text table: row i tests the
// UTF-8 of term ids[i] (bytes[offsets[id] .. offsets[id+1])) against one
// constant needle.  Output per row: 0 = no match, 1 = match, 2 = undecided
// (case folding met a non-ASCII byte before the row was decided; the host
// resolves those with Python's Unicode rules).
enum StrMode : int32_t { SM_STARTS = 0, SM_ENDS, SM_CONTAINS, SM_EQUALS };
enum StrFold : int32_t { SF_NONE = 0, SF_LOWER, SF_UPPER };

constexpr int kStrMaxNeedle = 255;
constexpr int kStrNeedleQ = 32;        // needle staged as 32 qwords of LDS
// CONTAINS rows whose term is longer than this leave the one-lane-per-row
// kernel for the one-wave-per-term kernel.  Measured on an MI355X over
// 10M rows (profiles/strfilter_measurements.md): a full scan (needle that
// never matches) is flat within 2-7% for 128..512 B and degrades on either
// side (lower: atomics + second launch for rows one lane handles well;
// higher: one lane scans while 63 idle); with an early match the larger
// value wins, so 512.
constexpr int64_t kStrLongThreshold = 512;
constexpr int kStrLongGrid = 1024;     // fixed grid of the long-term launch
constexpr uint64_t kHiBits = 0x8080808080808080ull;

// Aligned 8-byte load of qword q of the text blob.  `cap` is the blob's byte
// count: a trailing partial qword is assembled bytewise and anything past
// it reads as zero, so no lane ever touches memory outside [0, cap).
__device__ __forceinline__ uint64_t str_ld_q(const uint8_t* __restrict__ bytes,
                                             int64_t q, int64_t cap) {
  if (q < 0) return 0;
  if ((q + 1) * 8 <= cap)
    return reinterpret_cast<const uint64_t*>(bytes)[q];
  uint64_t v = 0;
  for (int64_t b = q * 8; b < cap; ++b)
    v |= static_cast<uint64_t>(bytes[b]) << (8 * (b - q * 8));
  return v;
}

// 8 bytes starting at arbitrary byte position p, from two aligned loads.
__device__ __forceinline__ uint64_t str_window(const uint8_t* __restrict__ bytes,
                                               int64_t p, int64_t cap) {
  int64_t q = p >> 3;
  int sh = static_cast<int>(p & 7) * 8;
  uint64_t lo = str_ld_q(bytes, q, cap);
  if (sh == 0) return lo;
  uint64_t hi = str_ld_q(bytes, q + 1, cap);
  return (lo >> sh) | (hi << (64 - sh));
}

// mask of the low k bytes (k >= 8 -> all)
__device__ __forceinline__ uint64_t str_byte_mask(int64_t k) {
  return k >= 8 ? ~0ull : ((1ull << (8 * k)) - 1ull);
}

// SWAR ASCII case fold of 8 bytes; bytes >= 0x80 pass through unchanged.
__device__ __forceinline__ uint64_t str_fold_q(uint64_t x, int32_t fold) {
  if (fold == SF_NONE) return x;
  uint64_t x7 = x & 0x7f7f7f7f7f7f7f7full;
  uint64_t ge_lo, gt_hi;
  if (fold == SF_LOWER) {            // 'A'(0x41) .. 'Z'(0x5a)
    ge_lo = x7 + 0x3f3f3f3f3f3f3f3full;
    gt_hi = x7 + 0x2525252525252525ull;
  } else {                           // 'a'(0x61) .. 'z'(0x7a)
    ge_lo = x7 + 0x1f1f1f1f1f1f1f1full;
    gt_hi = x7 + 0x0505050505050505ull;
  }
  uint64_t letter = ge_lo & ~gt_hi & ~x & kHiBits;
  return x ^ (letter >> 2);          // flip bit 0x20 of each letter
}

// any byte >= 0x80 in [start, end)?
__device__ __forceinline__ bool str_has_high(const uint8_t* __restrict__ bytes,
                                             int64_t start, int64_t end,
                                             int64_t cap) {
  for (int64_t p = start; p < end; p += 8)
    if (str_window(bytes, p, cap) & str_byte_mask(end - p) & kHiBits)
      return true;
  return false;
}

// needle[0..m) against the (folded) bytes at p: 1 match, 0 mismatch, 2 met a
// non-ASCII byte under folding before any mismatch.  Chunks before a
// mismatch are pure ASCII, so for a window anchored at its FRONT (or an
// interior CONTAINS candidate, where a 0 only means "not here") a 0 holds
// under Unicode folding as well.  A back-anchored caller (ENDS) must rule
// out non-ASCII bytes in the whole window first.
__device__ __forceinline__ int str_cmp_at(const uint8_t* __restrict__ bytes,
                                          int64_t p, int64_t cap,
                                          const uint64_t* needle_q, int m,
                                          int32_t fold) {
  for (int k = 0; k < m; k += 8) {
    uint64_t t = str_window(bytes, p + k, cap);
    uint64_t mask = str_byte_mask(m - k);
    if (fold != SF_NONE) {
      if (t & mask & kHiBits) return 2;
      t = str_fold_q(t, fold);
    }
    if ((t ^ needle_q[k >> 3]) & mask) return 0;
  }
  return 1;
}

// Short-term kernel: one lane per row.  CONTAINS rows with a long term are
// appended to the overflow list instead of being scanned here.
__global__ void str_match_rows(const int32_t* __restrict__ ids, int64_t n,
                               const uint8_t* __restrict__ bytes, int64_t cap,
                               const int64_t* __restrict__ offsets, int64_t V,
                               const uint64_t* __restrict__ needle, int m,
                               int32_t mode, int32_t fold,
                               uint8_t* __restrict__ out,
                               int32_t* __restrict__ ovf_count,
                               int32_t* __restrict__ ovf_rows) {
  __shared__ uint64_t s_needle[kStrNeedleQ];
  if (threadIdx.x < kStrNeedleQ) s_needle[threadIdx.x] = needle[threadIdx.x];
  __syncthreads();
  for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    int32_t id = ids[row];
    uint8_t r = 0;
    if (id >= 0 && id < V) {       // unbound, quoted and unknown ids: 0
      int64_t start = offsets[id];
      int64_t end = offsets[id + 1];
      int64_t len = end - start;
      if (start < 0 || len < 0 || end > cap) {
        r = 0;                     // corrupt table: never read it
      } else if (m == 0) {
        r = (mode == SM_EQUALS) ? (len == 0) : 1;
      } else if (len < m) {
        // a folded non-ASCII term may grow (UCASE("ß") = "SS")
        r = (fold != SF_NONE && str_has_high(bytes, start, end, cap)) ? 2 : 0;
      } else if (mode == SM_EQUALS && len != m) {
        // a character of <= 4 bytes folds to >= 1 character, so only terms
        // up to 4*m bytes can fold down to m characters
        r = (fold != SF_NONE && len <= 4 * (int64_t)m
             && str_has_high(bytes, start, end, cap)) ? 2 : 0;
      } else if (mode != SM_CONTAINS) {
        int64_t w0 = (mode == SM_ENDS) ? end - m : start;
        // STARTS / EQUALS are front-aligned: the ASCII chunks before a
        // mismatch fold 1:1, so str_cmp_at's early 0 is final.  ENDS is
        // back-aligned: a character later in the window whose fold changes
        // its byte length ("ı" -> "I", U+212A -> "k") shifts the folded
        // suffix against the raw window, so no chunk may answer 0 before
        // the WHOLE window is known to be ASCII.
        if (mode == SM_ENDS && fold != SF_NONE
            && str_has_high(bytes, w0, end, cap))
          r = 2;
        else
          r = static_cast<uint8_t>(
              str_cmp_at(bytes, w0, cap, s_needle, m, fold));
      } else if (len > kStrLongThreshold) {
        int32_t slot = atomicAdd(ovf_count, 1);
        ovf_rows[slot] = static_cast<int32_t>(row);   // slot < n by count
        r = 0;
      } else {
        // slide over every start position; the two aligned qwords under
        // the window are folded once on load and reused for 8 positions
        int64_t last = end - m;
        int64_t q = start >> 3;
        uint64_t lo = str_fold_q(str_ld_q(bytes, q, cap), fold);
        uint64_t hi = str_fold_q(str_ld_q(bytes, q + 1, cap), fold);
        uint64_t n0 = s_needle[0];
        uint64_t mask0 = str_byte_mask(m);
        bool found = false;
        for (int64_t p = start; p <= last; ++p) {
          int sh = static_cast<int>(p & 7) * 8;
          if (sh == 0 && p != start) {
            ++q;
            lo = hi;
            hi = str_fold_q(str_ld_q(bytes, q + 1, cap), fold);
          }
          uint64_t t = sh ? ((lo >> sh) | (hi << (64 - sh))) : lo;
          if (((t ^ n0) & mask0) == 0) {
            if (m <= 8 || str_cmp_at(bytes, p + 8, cap, s_needle + 1, m - 8,
                                     fold) == 1) {
              found = true;
              break;
            }
          }
        }
        // an all-ASCII match is final; a miss is final only if no byte of
        // the term could fold differently
        if (found) r = 1;
        else r = (fold != SF_NONE && str_has_high(bytes, start, end, cap))
                     ? 2 : 0;
      }
    }
    out[row] = r;
  }
}

// Long-term kernel: one wave per overflow row, lanes take consecutive start
// positions, a ballot combines them.  Fixed grid; the row count is read
// from device memory so the host never waits between the two launches.
__global__ void str_match_long(const int32_t* __restrict__ ids,
                               const uint8_t* __restrict__ bytes, int64_t cap,
                               const int64_t* __restrict__ offsets,
                               const uint64_t* __restrict__ needle, int m,
                               int32_t fold, uint8_t* __restrict__ out,
                               const int32_t* __restrict__ ovf_count,
                               const int32_t* __restrict__ ovf_rows) {
  __shared__ uint64_t s_needle[kStrNeedleQ];
  if (threadIdx.x < kStrNeedleQ) s_needle[threadIdx.x] = needle[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t count = *ovf_count;
  for (int64_t w = wave; w < count; w += n_waves) {   // wave-uniform
    int32_t row = ovf_rows[w];
    int32_t id = ids[row];
    int64_t start = offsets[id];
    int64_t end = offsets[id + 1];
    int64_t last = end - m;
    bool found = false;
    for (int64_t base = start; base <= last; base += 64) {
      int64_t p = base + lane;
      bool hit = p <= last
                 && str_cmp_at(bytes, p, cap, s_needle, m, fold) == 1;
      if (__ballot(hit) != 0ull) { found = true; break; }
    }
    uint8_t r = 1;
    if (!found) {
      r = 0;
      if (fold != SF_NONE) {
        bool high = false;
        for (int64_t p = start + (int64_t)lane * 8; p < end; p += 512)
          high |= (str_window(bytes, p, cap) & str_byte_mask(end - p)
                   & kHiBits) != 0;
        if (__ballot(high) != 0ull) r = 2;
      }
    }
    if (lane == 0) out[row] = r;
  }
}

// ------------------------------------------------------ K11 term_order kernels
// ORDER BY collation over the device term-text table.  Python orders str by
// code point and UTF-8 byte order is code-point order, so a bytewise order of
// the term text is the order sorted() gives.  The host side
// (engine/collation.py) refines groups of terms most-significant-bytes first;
// these kernels supply one round's sort keys, the common-prefix skip and the
// numeric-vs-lexical classification.  One lane per element; text is read
// only through str_window / str_ld_q; an id outside [0, V) (unbound, quoted,
// past the vocabulary) or with a corrupt table entry is the empty string.
constexpr int64_t kLcpSentinel = int64_t(1) << 62;

// start byte and byte length of term `id`, (0, 0) for anything unreadable
__device__ __forceinline__ void term_span(int32_t id, int64_t V,
                                          const int64_t* __restrict__ offsets,
                                          int64_t cap, int64_t* start,
                                          int64_t* len) {
  *start = 0;
  *len = 0;
  if (id < 0 || id >= V) return;
  int64_t s = offsets[id];
  int64_t e = offsets[id + 1];
  if (s < 0 || e < s || e > cap) return;
  *start = s;
  *len = e - s;
}

// bytes left in a term of `len` bytes from byte `depth` on (0 when past it)
__device__ __forceinline__ int64_t term_rest(int64_t len, int64_t depth) {
  if (depth < 0) depth = 0;
  return depth >= len ? 0 : len - depth;
}

// Sort key of the 7 bytes at depth[i]: bytes big-endian in bits 63..8 (zeros
// past the term's end), count of real bytes (0..7) in the low byte, sign bit
// flipped so a SIGNED sort orders the keys as unsigned.  The count byte puts
// a term before every longer term it is a prefix of, NUL bytes included.
__global__ void term_chunk_keys_kernel(const int32_t* __restrict__ ids,
                                       const int64_t* __restrict__ depth,
                                       int64_t m,
                                       const uint8_t* __restrict__ bytes,
                                       int64_t cap,
                                       const int64_t* __restrict__ offsets,
                                       int64_t V, int64_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t start, len;
    term_span(ids[i], V, offsets, cap, &start, &len);
    int64_t d = depth[i];
    int64_t rest = term_rest(len, d);
    int64_t cnt = rest < 7 ? rest : 7;
    uint64_t key = 0;
    if (cnt > 0) {
      uint64_t w = str_window(bytes, start + d, cap) & str_byte_mask(cnt);
      key = __builtin_bswap64(w);    // byte 0 -> bits 63..56; byte 7 masked off
    }
    key |= static_cast<uint64_t>(cnt);
    out[i] = static_cast<int64_t>(key ^ 0x8000000000000000ull);
  }
}

// Common-prefix length of terms i-1 and i measured from depth[i], for rows
// with same_group[i]; the sentinel for row 0 and for group heads.
__global__ void term_adjacent_lcp_kernel(const int32_t* __restrict__ ids,
                                         const int64_t* __restrict__ depth,
                                         const bool* __restrict__ same_group,
                                         int64_t m,
                                         const uint8_t* __restrict__ bytes,
                                         int64_t cap,
                                         const int64_t* __restrict__ offsets,
                                         int64_t V,
                                         int64_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i == 0 || !same_group[i]) {
      out[i] = kLcpSentinel;
      continue;
    }
    int64_t sa, la, sb, lb;
    term_span(ids[i - 1], V, offsets, cap, &sa, &la);
    term_span(ids[i], V, offsets, cap, &sb, &lb);
    int64_t d = depth[i];
    if (d < 0) d = 0;
    int64_t ra = term_rest(la, d);
    int64_t rb = term_rest(lb, d);
    int64_t lim = ra < rb ? ra : rb;
    int64_t k = 0;
    for (; k < lim; k += 8) {
      uint64_t x = (str_window(bytes, sa + d + k, cap)
                    ^ str_window(bytes, sb + d + k, cap))
                   & str_byte_mask(lim - k);
      if (x) {
        k += __builtin_ctzll(x) >> 3;
        break;
      }
    }
    out[i] = k < lim ? k : lim;
  }
}

// Decimal-literal automaton for [+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?
enum NumState : int {
  NS_START = 0, NS_SIGN, NS_INT, NS_DOT, NS_FRAC, NS_E, NS_ESIGN, NS_EXP,
  NS_DEAD
};

__device__ __forceinline__ int num_step(int st, uint8_t b) {
  bool digit = b >= '0' && b <= '9';
  bool sign = b == '+' || b == '-';
  bool dot = b == '.';
  bool e = b == 'e' || b == 'E';
  switch (st) {
    case NS_START: return digit ? NS_INT : sign ? NS_SIGN : dot ? NS_DOT
                                                                : NS_DEAD;
    case NS_SIGN:  return digit ? NS_INT : dot ? NS_DOT : NS_DEAD;
    case NS_INT:   return digit ? NS_INT : dot ? NS_FRAC : e ? NS_E : NS_DEAD;
    case NS_DOT:   return digit ? NS_FRAC : NS_DEAD;
    case NS_FRAC:  return digit ? NS_FRAC : e ? NS_E : NS_DEAD;
    case NS_E:     return digit ? NS_EXP : sign ? NS_ESIGN : NS_DEAD;
    case NS_ESIGN: return digit ? NS_EXP : NS_DEAD;
    case NS_EXP:   return digit ? NS_EXP : NS_DEAD;
    default:       return NS_DEAD;
  }
}

// a printable ASCII byte that no string accepted by Python's float() holds
__device__ __forceinline__ bool num_forbidden(uint8_t b) {
  if (b < 0x21 || b > 0x7e) return false;
  if (b >= '0' && b <= '9') return false;
  switch (b) {
    case '+': case '-': case '.': case '_':
    case 'e': case 'a': case 'f': case 'i': case 'n': case 't': case 'y':
    case 'E': case 'A': case 'F': case 'I': case 'N': case 'T': case 'Y':
      return false;
    default:
      return true;
  }
}

// 1 = the whole term is a decimal literal (float() accepts), 0 = empty,
// unreadable id or a forbidden byte (float() rejects), 2 = undecided: the
// host applies Python's own rules (padding, underscores, nan/inf, non-ASCII
// digits).
__global__ void term_numeric_class_kernel(const int32_t* __restrict__ ids,
                                          int64_t m,
                                          const uint8_t* __restrict__ bytes,
                                          int64_t cap,
                                          const int64_t* __restrict__ offsets,
                                          int64_t V,
                                          uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t start, len;
    term_span(ids[i], V, offsets, cap, &start, &len);
    if (len == 0) {
      out[i] = 0;
      continue;
    }
    int st = NS_START;
    bool forbidden = false;
    for (int64_t p = 0; p < len && !forbidden; p += 8) {
      uint64_t w = str_window(bytes, start + p, cap);
      int nb = len - p < 8 ? static_cast<int>(len - p) : 8;
      for (int k = 0; k < nb; ++k) {
        uint8_t b = static_cast<uint8_t>(w >> (8 * k));
        st = num_step(st, b);
        if (num_forbidden(b)) {
          forbidden = true;
          break;
        }
      }
    }
    bool accept = st == NS_INT || st == NS_FRAC || st == NS_EXP;
    out[i] = forbidden ? 0 : accept ? 1 : 2;
  }
}

// ------------------------------------------------------ K12 path_reach kernels
// Reachability from up to 64 sources at once over a CSR adjacency of compact
// node ids (p+ / p* / p? from a bound endpoint).  Source k of a pass owns bit
// k of three per-node uint64 masks: `seen` (reached by a path of >= 1 edge),
// `cur` (this level's frontier) and `nxt` (the next one).  Sources are NOT
// pre-marked in seen, so a source reaches itself only round a cycle.
//
// One launch is one BFS level over a node-id work queue whose length lives in
// device memory; the grid is fixed and strides over that length, so a level
// on an empty queue is a no-op and the host may launch several levels back to
// back before it reads the length once.  Words of the pass state:
//   [0..2] queue lengths in rotation: level k reads [k%3], appends to
//          [(k+1)%3] and zeroes [(k+2)%3] (last level's input, next level's
//          output: no block touches it during level k)
//   [3]    levels that found a non-empty queue
//   [4]    appends refused because the queue was full (never, by the
//          once-per-level rule below; the host raises if it is not 0)
// Blocks of one launch share data only through atomics: seen/nxt take
// agent-scope 64-bit ORs, the queue length an add.  The plain load of
// seen[w] in front of the OR is a filter only: an L1/L2 copy can be stale
// towards FEWER bits (bits are only ever added inside a pass), which costs a
// redundant atomic and never loses one.  A node enters the next queue only
// when nxt[w] was 0 before the OR, so at most once per level: n_nodes
// entries suffice.  cur[v] is cleared by the one lane that owns queue entry
// v, so the array is all zero when it becomes `nxt` two levels on.
constexpr int kReachBlock = 256;
constexpr int kReachGrid = 1024;       // 4 blocks per CU, strides the queue
constexpr int kReachStateWords = 8;
constexpr int kReachBatch = 64;        // sources per pass = mask bits

__device__ __forceinline__ uint64_t reach_shfl64(uint64_t x, int src) {
  uint32_t lo = __shfl(static_cast<uint32_t>(x), src);
  uint32_t hi = __shfl(static_cast<uint32_t>(x >> 32), src);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// offer mask m to neighbour w; true when w must join the next queue
__device__ __forceinline__ bool reach_visit(
    int32_t w, uint64_t m, int32_t n_nodes,
    unsigned long long* __restrict__ seen,
    unsigned long long* __restrict__ nxt) {
  if (static_cast<uint32_t>(w) >= static_cast<uint32_t>(n_nodes)) return false;
  uint64_t d = m & ~seen[w];
  if (d == 0) return false;
  d &= ~atomicOr(&seen[w], d);
  if (d == 0) return false;
  return atomicOr(&nxt[w], d) == 0;
}

// wave-aggregated queue append (guide G12): one add per wave instruction.
// Must be reached by all 64 lanes.
__device__ __forceinline__ void reach_push(bool push, int32_t w, int lane,
                                           int32_t* __restrict__ q_out,
                                           uint32_t* len_out, uint32_t cap,
                                           uint32_t* refused) {
  const uint64_t b = __ballot(push);
  if (b == 0) return;
  const int leader = __ffsll(static_cast<unsigned long long>(b)) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(len_out, static_cast<uint32_t>(__popcll(b)));
  base = __shfl(base, leader);
  if (push) {
    uint32_t pos = base + __popcll(b & ((1ull << lane) - 1ull));
    if (pos < cap) q_out[pos] = w;
    else atomicAdd(refused, 1u);
  }
}

__global__ void path_reach_seed(const int32_t* __restrict__ sources, int n_src,
                                int32_t n_nodes,
                                unsigned long long* __restrict__ cur,
                                int32_t* __restrict__ queue,
                                uint32_t* __restrict__ state) {
  const int k = threadIdx.x;
  if (k >= n_src) return;
  const int32_t v = sources[k];
  if (static_cast<uint32_t>(v) >= static_cast<uint32_t>(n_nodes)) return;
  // the same node may be the source of several bits: queue it once
  if (atomicOr(&cur[v], 1ull << k) == 0) {
    uint32_t pos = atomicAdd(&state[0], 1u);
    queue[pos] = v;                     // pos < n_src <= 64 <= queue capacity
  }
}

__global__ void __launch_bounds__(kReachBlock)
path_reach_level(const int32_t* __restrict__ row_ptr,
                 const int32_t* __restrict__ col, int32_t n_nodes,
                 unsigned long long* __restrict__ seen,
                 unsigned long long* __restrict__ cur,
                 unsigned long long* __restrict__ nxt,
                 const int32_t* __restrict__ q_in, int32_t* __restrict__ q_out,
                 uint32_t* state, int slot, int hub_degree) {
  const int lane = threadIdx.x & 63;
  const uint32_t len_in = state[slot];
  uint32_t* len_out = &state[(slot + 1) % 3];
  uint32_t* refused = &state[4];
  const uint32_t cap = static_cast<uint32_t>(n_nodes);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state[(slot + 2) % 3] = 0;
    if (len_in != 0) state[3] += 1;
  }
  const uint32_t wave = (blockIdx.x * kReachBlock + threadIdx.x) >> 6;
  const uint32_t n_waves = gridDim.x * (kReachBlock >> 6);
  // A wave takes `chunk` consecutive entries per trip: 64 when the queue
  // fills the grid, fewer when it is short, so that the entries of a short
  // queue (64 hubs, say) go to as many waves instead of queueing up in one.
  // Wave-uniform trip count: the ballots below need all 64 lanes.
  uint32_t chunk = (len_in + n_waves - 1) / n_waves;
  chunk = chunk < 1 ? 1 : chunk > 64 ? 64 : chunk;
  for (uint64_t base = static_cast<uint64_t>(wave) * chunk; base < len_in;
       base += static_cast<uint64_t>(n_waves) * chunk) {
    const uint64_t i = base + lane;
    const bool act = static_cast<uint32_t>(lane) < chunk && i < len_in;
    uint64_t m = 0;
    int32_t rs = 0, re = 0;
    if (act) {
      const int32_t v = q_in[i];
      if (static_cast<uint32_t>(v) < cap) {
        m = cur[v];
        cur[v] = 0;
        rs = row_ptr[v];
        re = row_ptr[v + 1];
      }
    }
    const int deg = re - rs;
    const bool hub = deg >= hub_degree;
    // tier 1: a lane walks its own short neighbour list
    const int mine = hub ? 0 : deg;
    for (int j = 0; __any(j < mine); ++j) {
      bool push = false;
      int32_t w = 0;
      if (j < mine) {
        w = col[rs + j];
        push = reach_visit(w, m, n_nodes, seen, nxt);
      }
      reach_push(push, w, lane, q_out, len_out, cap, refused);
    }
    // tier 2: the wave walks each long list together, coalesced col reads
    uint64_t hubs = __ballot(hub);
    while (hubs != 0) {
      const int src = __ffsll(static_cast<unsigned long long>(hubs)) - 1;
      hubs &= hubs - 1;
      const int64_t hs = __shfl(rs, src);
      const int64_t he = __shfl(re, src);
      const uint64_t hm = reach_shfl64(m, src);
      for (int64_t e = hs; e < he; e += 64) {
        const int64_t idx = e + lane;
        bool push = false;
        int32_t w = 0;
        if (idx < he) {
          w = col[idx];
          push = reach_visit(w, hm, n_nodes, seen, nxt);
        }
        reach_push(push, w, lane, q_out, len_out, cap, refused);
      }
    }
  }
}

// Per node the number of sources that reached it, and per source (bit) the
// number of nodes it reached: lane k sums bit k, one add per lane and wave.
__global__ void __launch_bounds__(kReachBlock)
path_reach_count(const unsigned long long* __restrict__ seen, int32_t n_nodes,
                 int32_t* __restrict__ node_count,
                 unsigned long long* __restrict__ per_source) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * kReachBlock + threadIdx.x) >> 6;
  const uint32_t n_waves = gridDim.x * (kReachBlock >> 6);
  unsigned long long acc = 0;
  for (int64_t base = static_cast<int64_t>(wave) * 64; base < n_nodes;
       base += static_cast<int64_t>(n_waves) * 64) {
    const int64_t v = base + lane;
    const uint64_t m = v < n_nodes ? seen[v] : 0;
    if (v < n_nodes && node_count != nullptr) node_count[v] = __popcll(m);
    if (__ballot(m != 0) == 0) continue;
    for (int k = 0; k < 64; ++k) {
      const uint64_t b = __ballot((m >> k) & 1);
      if (lane == k) acc += __popcll(b);
    }
  }
  if (acc != 0) atomicAdd(&per_source[lane], acc);
}

// did source k reach itself (it lies on a cycle)?
__global__ void path_reach_self(const int32_t* __restrict__ sources, int n_src,
                                int32_t n_nodes,
                                const unsigned long long* __restrict__ seen,
                                uint8_t* __restrict__ self_hit) {
  const int k = threadIdx.x;
  if (k >= n_src) return;
  const int32_t v = sources[k];
  bool hit = false;
  if (static_cast<uint32_t>(v) < static_cast<uint32_t>(n_nodes))
    hit = (seen[v] >> k) & 1;
  self_hit[k] = hit ? 1 : 0;
}

// (source position, node) per set bit, at the node's exclusive-scan offset
__global__ void __launch_bounds__(kReachBlock)
path_reach_emit(const unsigned long long* __restrict__ seen, int32_t n_nodes,
                const int64_t* __restrict__ offset_incl,
                int32_t pos_base, int64_t total,
                int32_t* __restrict__ out_pos, int32_t* __restrict__ out_node) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n_nodes;
       v += (int64_t)gridDim.x * blockDim.x) {
    uint64_t m = seen[v];
    if (m == 0) continue;
    int64_t at = offset_incl[v] - __popcll(m);
    while (m != 0) {
      const int k = __ffsll(static_cast<unsigned long long>(m)) - 1;
      m &= m - 1;
      if (at >= 0 && at < total) {
        out_pos[at] = pos_base + k;
        out_node[at] = static_cast<int32_t>(v);
      }
      ++at;
    }
  }
}

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

}  // namespace

// --------------------------------------------- fused chain-count (K1+K2+K4)
// COUNT(*) over a probe chain whose hop keys all come from the SEED scan:
//   count = sum over seed rows of prod_h |matches_h(key_h(row))|
// One kernel, no intermediate materialization.  Hop regions are
// pre-narrowed to their predicate slice on the host.
constexpr int kMaxHops = 4;

struct ChainHops {
  // narrowed sorted regions, stored as the 32-bit LOW components only
  // (the high word is the hop's constant predicate — dropping it halves
  // the streamed bytes and doubles the LDS window capacity); ascending in
  // UNSIGNED 32-bit order, so all searches compare as uint32
  const int32_t* key32[kMaxHops];
  int64_t n[kMaxHops];
  int32_t src[kMaxHops];           // 0: seed B component, 1: seed Z column
  const unsigned long long* table[kMaxHops];  // optional count table (u64)
  const uint32_t* table32[kMaxHops];  // packed (val<<7)|count u32 variant
  // DIRECT-indexed count table (dense value spaces, e.g. a contiguous
  // id block): counts[v - dmin] — consecutive seed values hit
  // consecutive slots, so the probe loads COALESCE instead of hashing
  // to random lines
  const uint32_t* direct[kMaxHops];
  int64_t dmin[kMaxHops];
  int64_t dlen[kMaxHops];
  int64_t tmask[kMaxHops];
  int k;
  // stage a window through LDS only when it exceeds this row count:
  // small windows (few cache lines, shared by the whole block) search
  // L1/L2 directly without the staging barrier
  int lds_min = 0;
};

__device__ __forceinline__ int64_t lower_bound_u32(
    const int32_t* __restrict__ a, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (static_cast<uint32_t>(a[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t upper_bound_u32(
    const int32_t* __restrict__ a, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (static_cast<uint32_t>(a[mid]) <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// packed-u32 count table: halves the table footprint (better L2 residency
// beside the seed stream) when every value < 2^25 and count < 2^7
constexpr uint32_t kTbl32Empty = 0xFFFFFFFFu;

// ---- per-hop COUNT tables -------------------------------------------------
// A small hop region (e.g. the 142k-row locatedIn slice under 14.2M seeds)
// makes every seed pay a ~17-level binary search = ~17 distinct L2 lines.
// Instead the host collapses the region to (value, count) pairs once per
// store version and an open-addressing table turns the hop into ONE 8-byte
// L2 load (entry packed (val<<32)|count, empty slot = all-ones).
constexpr unsigned long long kTblEmpty = ~0ull;

__device__ __forceinline__ uint32_t h32(uint32_t x) {
  x *= 2654435761u;
  x ^= x >> 16;
  return x;
}

// ---- K8: database statistics gather ---------------------------------------
// One pass over the committed (s, p, o) columns computes everything the
// cost model needs: per-predicate row counts, global distinct
// subjects/objects, and per-predicate distinct subjects/objects (as
// (p,x) pair claims).  Presence tables are open-addressing claims
// (atomicCAS); row counts aggregate through a per-block LDS histogram
// (predicate sets are tiny); distinct tallies use per-thread
// accumulators folded by one wave reduction (guide G12).
// Ref parity: streamertail_optimizer/stats/database_stats.rs:18-158.
constexpr int kStatsPreds = 1024;  // open-addressing predicate slots
constexpr uint32_t kStatsEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ int stats_pred_slot(uint32_t* pred_keys,
                                               uint32_t pkey) {
  uint32_t slot = h32(pkey) & (kStatsPreds - 1);
  for (;;) {
    uint32_t cur = __hip_atomic_load(&pred_keys[slot], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    if (cur == pkey) return static_cast<int>(slot);
    if (cur == kStatsEmpty) {
      uint32_t prev = atomicCAS(&pred_keys[slot], kStatsEmpty, pkey);
      if (prev == kStatsEmpty || prev == pkey)
        return static_cast<int>(slot);
      continue;  // lost the race to a different key: re-inspect the slot
    }
    slot = (slot + 1) & (kStatsPreds - 1);
  }
}

__device__ __forceinline__ bool stats_claim_u32(uint32_t* tbl, uint32_t mask,
                                                uint32_t v) {
  uint32_t slot = h32(v) & mask;
  for (;;) {
    uint32_t cur = __hip_atomic_load(&tbl[slot], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    if (cur == v) return false;
    if (cur == kStatsEmpty) {
      uint32_t prev = atomicCAS(&tbl[slot], kStatsEmpty, v);
      if (prev == kStatsEmpty) return true;
      if (prev == v) return false;
      continue;
    }
    slot = (slot + 1) & mask;
  }
}

__device__ __forceinline__ bool stats_claim_u64(unsigned long long* tbl,
                                                uint32_t mask,
                                                unsigned long long v) {
  uint32_t slot = h32(static_cast<uint32_t>(v)
                      ^ static_cast<uint32_t>(v >> 32)) & mask;
  for (;;) {
    unsigned long long cur = __hip_atomic_load(
        &tbl[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == v) return false;
    if (cur == ~0ull) {
      unsigned long long prev = atomicCAS(&tbl[slot], ~0ull, v);
      if (prev == ~0ull) return true;
      if (prev == v) return false;
      continue;
    }
    slot = (slot + 1) & mask;
  }
}

__global__ void stats_gather_kernel(
    const int32_t* __restrict__ s, const int32_t* __restrict__ p,
    const int32_t* __restrict__ o, int64_t n, uint32_t* pred_keys,
    unsigned long long* pred_rows, unsigned long long* pred_ds,
    unsigned long long* pred_do, uint32_t* s_tbl, uint32_t* o_tbl,
    uint32_t so_mask, unsigned long long* ps_tbl,
    unsigned long long* po_tbl, uint32_t pair_mask,
    unsigned long long* g_counts /* [0]=distinct_s [1]=distinct_o */) {
  __shared__ uint32_t lds_rows[kStatsPreds];
  for (int i = threadIdx.x; i < kStatsPreds; i += blockDim.x)
    lds_rows[i] = 0;
  __syncthreads();
  unsigned long long acc_s = 0, acc_o = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t pp = static_cast<uint32_t>(p[i]);
    uint32_t ss = static_cast<uint32_t>(s[i]);
    uint32_t oo = static_cast<uint32_t>(o[i]);
    int slot = stats_pred_slot(pred_keys, pp);
    atomicAdd(&lds_rows[slot], 1u);
    if (stats_claim_u32(s_tbl, so_mask, ss)) ++acc_s;
    if (stats_claim_u32(o_tbl, so_mask, oo)) ++acc_o;
    unsigned long long base = static_cast<unsigned long long>(pp) << 32;
    if (stats_claim_u64(ps_tbl, pair_mask, base | ss))
      atomicAdd(&pred_ds[slot], 1ull);
    if (stats_claim_u64(po_tbl, pair_mask, base | oo))
      atomicAdd(&pred_do[slot], 1ull);
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc_s += __shfl_down(acc_s, off);
    acc_o += __shfl_down(acc_o, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (acc_s) atomicAdd(&g_counts[0], acc_s);
    if (acc_o) atomicAdd(&g_counts[1], acc_o);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kStatsPreds; i += blockDim.x)
    if (lds_rows[i])
      atomicAdd(&pred_rows[i], static_cast<unsigned long long>(lds_rows[i]));
}

std::vector<at::Tensor> stats_gather(at::Tensor s, at::Tensor p,
                                     at::Tensor o) {
  TORCH_CHECK(s.is_cuda() && p.is_cuda() && o.is_cuda(),
              "stats_gather: device columns required");
  TORCH_CHECK(s.dtype() == at::kInt && p.dtype() == at::kInt
              && o.dtype() == at::kInt);
  int64_t n = s.numel();
  TORCH_CHECK(p.numel() == n && o.numel() == n);
  int64_t so_size = 64;
  while (so_size < 2 * n) so_size <<= 1;
  auto opt_i = s.options();
  auto opt_l = s.options().dtype(at::kLong);
  auto pred_keys = at::full({kStatsPreds}, -1, opt_i);
  auto pred_rows = at::zeros({kStatsPreds}, opt_l);
  auto pred_ds = at::zeros({kStatsPreds}, opt_l);
  auto pred_do = at::zeros({kStatsPreds}, opt_l);
  auto s_tbl = at::full({so_size}, -1, opt_i);
  auto o_tbl = at::full({so_size}, -1, opt_i);
  auto ps_tbl = at::full({so_size}, -1, opt_l);
  auto po_tbl = at::full({so_size}, -1, opt_l);
  auto g_counts = at::zeros({2}, opt_l);
  if (n > 0) {
    hipLaunchKernelGGL(
        stats_gather_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
        cur_stream(), s.data_ptr<int32_t>(), p.data_ptr<int32_t>(),
        o.data_ptr<int32_t>(),
        n, reinterpret_cast<uint32_t*>(pred_keys.data_ptr<int32_t>()),
        reinterpret_cast<unsigned long long*>(pred_rows.data_ptr<int64_t>()),
        reinterpret_cast<unsigned long long*>(pred_ds.data_ptr<int64_t>()),
        reinterpret_cast<unsigned long long*>(pred_do.data_ptr<int64_t>()),
        reinterpret_cast<uint32_t*>(s_tbl.data_ptr<int32_t>()),
        reinterpret_cast<uint32_t*>(o_tbl.data_ptr<int32_t>()),
        static_cast<uint32_t>(so_size - 1),
        reinterpret_cast<unsigned long long*>(ps_tbl.data_ptr<int64_t>()),
        reinterpret_cast<unsigned long long*>(po_tbl.data_ptr<int64_t>()),
        static_cast<uint32_t>(so_size - 1),
        reinterpret_cast<unsigned long long*>(g_counts.data_ptr<int64_t>()));
    HIP_OK(hipGetLastError());
  }
  return {pred_keys, pred_rows, pred_ds, pred_do, g_counts};
}


__global__ void count_table_insert(const int64_t* __restrict__ entries,
                                   int64_t u,
                                   unsigned long long* __restrict__ table,
                                   uint32_t mask) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < u;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long e = static_cast<unsigned long long>(entries[i]);
    uint32_t slot = h32(static_cast<uint32_t>(e >> 32)) & mask;
    while (atomicCAS(&table[slot], kTblEmpty, e) != kTblEmpty)
      slot = (slot + 1) & mask;
  }
}

__global__ void count_table_insert32(const int32_t* __restrict__ entries,
                                     int64_t u,
                                     uint32_t* __restrict__ table,
                                     uint32_t mask) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < u;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t e = static_cast<uint32_t>(entries[i]);
    uint32_t slot = h32(e >> 7) & mask;
    while (atomicCAS(&table[slot], kTbl32Empty, e) != kTbl32Empty)
      slot = (slot + 1) & mask;
  }
}

at::Tensor build_count_table32(at::Tensor packed_entries) {
  TORCH_CHECK(packed_entries.is_cuda()
              && packed_entries.dtype() == at::kInt);
  int64_t u = packed_entries.numel();
  int64_t size = 64;
  while (size < 2 * u) size <<= 1;
  auto table = at::full({size}, -1, packed_entries.options());
  if (u > 0) {
    hipLaunchKernelGGL(count_table_insert32, dim3(grid_for(u)), dim3(kBlock),
                       0, cur_stream(), packed_entries.data_ptr<int32_t>(),
                       u,
                       reinterpret_cast<uint32_t*>(
                           table.data_ptr<int32_t>()),
                       static_cast<uint32_t>(size - 1));
    HIP_OK(hipGetLastError());
  }
  return table;
}

at::Tensor build_count_table(at::Tensor packed_entries) {
  TORCH_CHECK(packed_entries.is_cuda()
              && packed_entries.dtype() == at::kLong);
  int64_t u = packed_entries.numel();
  int64_t size = 64;
  while (size < 2 * u) size <<= 1;
  auto table = at::full({size}, -1, packed_entries.options());
  if (u > 0) {
    hipLaunchKernelGGL(count_table_insert, dim3(grid_for(u)), dim3(kBlock), 0,
                       cur_stream(), packed_entries.data_ptr<int64_t>(), u,
                       reinterpret_cast<unsigned long long*>(
                           table.data_ptr<int64_t>()),
                       static_cast<uint32_t>(size - 1));
    HIP_OK(hipGetLastError());
  }
  return table;
}

// The chain kernel's own tile: ONE WAVE owns kChainTile seeds, as
// kChainGroups groups of 256; in a group each lane owns kChainSeeds
// CONSECUTIVE seeds (one dwordx4 per seed column).  Nothing is shared
// between waves, so the kernel runs single-wave workgroups and needs no
// hardware barrier.  Separate from kTile, which the merge-path probes above
// share.
constexpr int kChainSeeds = 4;
constexpr int kChainWave = 64;
constexpr int kChainGroups = 4;
constexpr int kChainTile = kChainSeeds * kChainWave * kChainGroups;

// per-(tile, src0-hop) windows: the seed region is subject-sorted, so the
// B component is monotone — each kChainTile-seed tile's src-0 hop keys fall
// in a narrow window of that hop's region (merge-path; computed in
// parallel).
__global__ void chain_tile_bounds(const int32_t* __restrict__ seed_b,
                                  int64_t m, int64_t n_tiles, ChainHops hops,
                                  int64_t* __restrict__ win,  // [n_tiles][k][2]
                                  unsigned long long* __restrict__ total_zero
                                  ) {
  if (total_zero && blockIdx.x == 0 && threadIdx.x == 0)
    *total_zero = 0ULL;  // saves the serve path a hipMemsetAsync enqueue
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tiles;
       t += (int64_t)gridDim.x * blockDim.x) {
    uint32_t first_b = static_cast<uint32_t>(seed_b[t * kChainTile]);
    uint32_t last_b =
        static_cast<uint32_t>(seed_b[min((t + 1) * kChainTile - 1, m - 1)]);
    for (int h = 0; h < hops.k; ++h) {
      int64_t lo = 0, hi = hops.n[h];
      if (hops.table[h] != nullptr || hops.table32[h] != nullptr
          || hops.direct[h] != nullptr) {
        lo = hi = 0;  // hashed/direct hop: window unused
      } else if (hops.src[h] == 0) {
        lo = lower_bound_u32(hops.key32[h], hops.n[h], first_b);
        hi = upper_bound_u32(hops.key32[h], hops.n[h], last_b);
      }
      win[(t * hops.k + h) * 2] = lo;
      win[(t * hops.k + h) * 2 + 1] = hi;
    }
  }
}

// A tile's src-0 window holds exactly the region keys in [first, last], the
// tile's first and last seed keys.  The wave answers the hop from its own
// LDS slice of kChainSpan dwords, one of three ways (wave-uniform):
//   direct count  last - first < kChainSpan: hist[key - first] += 1 per
//                 window row (LDS atomic, no range check needed), then a
//                 seed's count is hist[b - first] — no search at all, and
//                 no row limit (rows beyond those loaded with the tile are
//                 streamed);
//   staged merge  the keys span more but the window has at most kChainSpan
//                 rows: stage the rows and merge in LDS;
//   global search anything else, and every window not above lds_min.
// 8 KB + pad per wave: 16 resident waves per CU (what the registers allow)
// take 129 of the 160 KB, so LDS does not lower residency.
constexpr int kChainSpan = 2048;
// partial sums the waves add their counts to, each on a 128-byte line of
// its own; chain_total_kernel folds them
constexpr int kChainParts = 256;
constexpr int kChainPartStride = 16;
// the 2 x b128 merge read may pass the window's end: the rows behind it
// hold kChainPadKey, which no key compares above (a seed equal to it is
// settled by the merge's search fallback)
constexpr int kChainPad = 8;
constexpr uint32_t kChainPadKey = 0xFFFFFFFFu;
// window rows per lane that are loaded with the tile's seeds (in registers):
// kChainPre * kChainWave rows, one tile's worth when keys and seeds are
// 1:1; the rest of a longer window is read when the tile is processed
constexpr int kChainPre = kChainTile / kChainWave;

enum ChainTier { kChainGlobal = 0, kChainMerge = 1, kChainDirect = 2 };

// everything a tile needs from global memory before its LDS work can
// start, loaded back to back
struct ChainTileIn {
  uint32_t b[kChainGroups][kChainSeeds], z[kChainGroups][kChainSeeds];
  uint32_t pw[kChainPre];
};

// one tile's window of one hop and the tile's first and last valid seed
// keys: wave-uniform, so they live in scalar registers
struct ChainWin {
  int64_t lo, span;
  uint32_t first, last;
};

__device__ __forceinline__ ChainWin chain_load_win(
    const int64_t* __restrict__ win, int64_t t, int k, int h, uint32_t first,
    uint32_t last) {
  ChainWin w{0, 0, first, last};
  if (h >= 0) {
    w.lo = win[(t * k + h) * 2];
    w.span = win[(t * k + h) * 2 + 1] - w.lo;
  }
  return w;
}

// `last - first`, not a span: that would wrap to 0 when the keys cover all
// of u32.  The direct count holds a window row count in 32 bits.
__device__ __forceinline__ int chain_tier(const ChainWin& w, int lds_min) {
  if (w.span <= 0 || w.span <= lds_min) return kChainGlobal;
  if (w.last - w.first < static_cast<uint32_t>(kChainSpan)
      && w.span <= 0xFFFFFFFFll)
    return kChainDirect;
  return w.span <= kChainSpan ? kChainMerge : kChainGlobal;
}

// one group's registers by a wave-uniform index.  Masks, not `?:` on the
// arrays: that becomes a selected address and sends them to scratch.
template <typename T>
__device__ __forceinline__ void chain_pick(
    const T (&a)[kChainGroups][kChainSeeds], int g, T (&out)[kChainSeeds]) {
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u) {
    T v = 0;
#pragma unroll
    for (int j = 0; j < kChainGroups; ++j)
      v |= a[j][u] & (g == j ? ~static_cast<T>(0) : static_cast<T>(0));
    out[u] = v;
  }
}

template <typename T>
__device__ __forceinline__ void chain_put(
    T (&a)[kChainGroups][kChainSeeds], int g, const T (&in)[kChainSeeds]) {
#pragma unroll
  for (int j = 0; j < kChainGroups; ++j) {
    T take = g == j ? ~static_cast<T>(0) : static_cast<T>(0);
#pragma unroll
    for (int u = 0; u < kChainSeeds; ++u)
      a[j][u] = (in[u] & take) | (a[j][u] & ~take);
  }
}

// a lane's kChainSeeds consecutive seeds of one column.  `vec` is
// wave-uniform: a full tile behind 16-byte aligned column pointers takes
// one dwordx4; the tail tile and unaligned columns (a slice of a larger
// tensor) take dword loads at a clamped index, nothing branching per seed;
// seeds past the end read as 0 and their contributions are dropped when the
// tile is summed.
template <bool kVec>
__device__ __forceinline__ void chain_load_seeds(
    const int32_t* __restrict__ col, int64_t i0, int64_t m,
    uint32_t (&out)[kChainSeeds]) {
  if (kVec) {
    uint4 v = *reinterpret_cast<const uint4*>(col + i0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int u = 0; u < kChainSeeds; ++u) {
      uint32_t v = static_cast<uint32_t>(col[min(i0 + u, m - 1)]);
      out[u] = i0 + u < m ? v : 0u;
    }
  }
}

// all seed and window loads of a tile, issued back to back
__device__ __forceinline__ void chain_load_tile(
    ChainTileIn& in, int64_t t, const int32_t* __restrict__ seed_b,
    const int32_t* __restrict__ seed_z, int64_t m, const ChainHops& hops,
    int hp, const ChainWin& w, bool vec) {
  if (__builtin_expect(vec && (t + 1) * kChainTile <= m, 1)) {
#pragma unroll
    for (int g = 0; g < kChainGroups; ++g) {
      int64_t i0 = t * kChainTile
          + (g * kChainWave + threadIdx.x) * kChainSeeds;
      chain_load_seeds<true>(seed_b, i0, m, in.b[g]);
      chain_load_seeds<true>(seed_z, i0, m, in.z[g]);
    }
  } else {
#pragma unroll
    for (int g = 0; g < kChainGroups; ++g) {
      int64_t i0 = t * kChainTile
          + (g * kChainWave + threadIdx.x) * kChainSeeds;
      chain_load_seeds<false>(seed_b, i0, m, in.b[g]);
      chain_load_seeds<false>(seed_z, i0, m, in.z[g]);
    }
  }
#pragma unroll
  for (int j = 0; j < kChainPre; ++j) in.pw[j] = 0;
  // the tier is known only once the seeds are here (it depends on their
  // first and last key), so the rows are fetched for every window that may
  // use the slice
  if (hp >= 0 && w.span > 0 && w.span > hops.lds_min) {
    const int32_t* base = hops.key32[hp] + w.lo + threadIdx.x;
    if (__builtin_expect(w.span >= kChainTile, 1)) {
#pragma unroll
      for (int j = 0; j < kChainPre; ++j)
        in.pw[j] = static_cast<uint32_t>(base[j * kChainWave]);
    } else {
      // rows past the window stay 0: they are skipped or replaced by the
      // pad key when the slice is filled
      int n = static_cast<int>(w.span) - static_cast<int>(threadIdx.x);
#pragma unroll
      for (int j = 0; j < kChainPre; ++j)
        if (j * kChainWave < n)
          in.pw[j] = static_cast<uint32_t>(base[j * kChainWave]);
    }
  }
}

// the tile's first and last valid seed key, from the registers that hold
// them (the keys chain_tile_bounds cut the windows by)
__device__ __forceinline__ void chain_tile_keys(const ChainTileIn& in,
                                                int64_t t, int64_t m,
                                                ChainWin& w) {
  int pos = static_cast<int>(
      min((t + 1) * kChainTile, m) - 1 - t * kChainTile);
  uint32_t at[kChainSeeds];
  chain_pick(in.b, pos / (kChainWave * kChainSeeds), at);
  uint32_t v = 0;
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u)
    v |= at[u] & ((pos & (kChainSeeds - 1)) == u ? 0xFFFFFFFFu : 0u);
  w.first = __builtin_amdgcn_readfirstlane(in.b[0][0]);
  w.last = __builtin_amdgcn_readlane(
      v, (pos / kChainSeeds) & (kChainWave - 1));
}

// The slice belongs to one wave, and a single-wave workgroup needs no
// hardware barrier: this only orders the wave's own LDS accesses (lanes
// read what other lanes wrote).
__device__ __forceinline__ void chain_wave_sync() { __syncthreads(); }

// stage window rows [r0 + lane, n) from global memory and the pad behind
// them
__device__ __forceinline__ void chain_stage_rows(
    uint32_t* lds, const int32_t* __restrict__ base, uint32_t n,
    uint32_t r0) {
  for (uint32_t r = r0 + threadIdx.x; r < n + kChainPad; r += kChainWave) {
    uint32_t v = kChainPadKey;
    if (r < n) v = static_cast<uint32_t>(base[r]);
    lds[r] = v;
  }
}

// direct count: zero hist[0, nkeys) with b128 stores (the slice is a
// multiple of 4 dwords, so rounding nkeys up stays inside it)
__device__ __forceinline__ void chain_hist_zero(uint32_t* lds,
                                                uint32_t nkeys) {
  for (uint32_t i = threadIdx.x * 4; i < nkeys; i += kChainWave * 4)
    *reinterpret_cast<uint4*>(lds + i) = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ void chain_hist_add(uint32_t* lds, uint32_t key,
                                               uint32_t first) {
  __hip_atomic_fetch_add(&lds[key - first], 1u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
}

// direct count: window rows [r0 + lane, n) streamed from global memory.
// Every row's key lies in [first, last], so no index is checked.
__device__ __forceinline__ void chain_hist_rows(
    uint32_t* lds, const int32_t* __restrict__ base, int64_t n, int64_t r0,
    uint32_t first) {
  for (int64_t r = r0 + threadIdx.x; r < n; r += kChainWave)
    chain_hist_add(lds, static_cast<uint32_t>(base[r]), first);
}

// direct count: a seed's count is its key's bin.  A seed past the end
// reads as 0: its index is clamped and its product dropped.
__device__ __forceinline__ void chain_hist_read(
    const uint32_t* lds, const uint32_t (&b)[kChainSeeds], uint32_t first,
    uint32_t last, unsigned long long (&prod)[kChainSeeds]) {
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u)
    prod[u] *= lds[min(b[u] - first, last - first)];
}

// fill the slice for one (tile, src-0 hop): the hop's histogram or its
// staged rows.  `pw` are the window's first kChainPre * kChainWave rows if
// they came with the tile's loads (pre), else everything is read here.
__device__ __forceinline__ void chain_fill_slice(
    uint32_t* lds, int tier, const int32_t* __restrict__ base,
    const ChainWin& w, const uint32_t (&pw)[kChainPre], bool pre) {
  uint32_t n = static_cast<uint32_t>(w.span);
  if (tier == kChainDirect) {
    chain_hist_zero(lds, w.last - w.first + 1);
    chain_wave_sync();
    if (pre && w.span >= kChainTile) {
#pragma unroll
      for (int j = 0; j < kChainPre; ++j) chain_hist_add(lds, pw[j], w.first);
    } else if (pre) {
#pragma unroll
      for (int j = 0; j < kChainPre; ++j)
        if (threadIdx.x + j * kChainWave < n)
          chain_hist_add(lds, pw[j], w.first);
    }
    chain_hist_rows(lds, base, w.span, pre ? kChainPre * kChainWave : 0,
                    w.first);
  } else {
    if (pre) {
#pragma unroll
      for (int j = 0; j < kChainPre; ++j) {
        uint32_t r = threadIdx.x + j * kChainWave;
        lds[r] = r < n ? pw[j] : kChainPadKey;
      }
    }
    chain_stage_rows(lds, base, n, pre ? kChainPre * kChainWave : 0);
  }
  chain_wave_sync();
}

// lower bound over a staged window (n >= 1) by bit descent: the largest
// pos with w[pos - 1] < key.  The trip count follows from the window size
// alone, so a wave stays converged; 32-bit indices throughout.
__device__ __forceinline__ uint32_t lds_lower_bound_fixed(
    const uint32_t* w, uint32_t n, uint32_t key) {
  uint32_t pos = 0;
  for (uint32_t step = 1u << (31 - __clz(static_cast<int>(n))); step > 0;
       step >>= 1) {
    uint32_t idx = pos + step;
    uint32_t v = w[min(idx, n) - 1];
    pos = (idx <= n) & (v < key) ? idx : pos;
  }
  return pos;
}

// plain bound in w[lo, hi) for the rare seeds the merge read cannot settle
__device__ __forceinline__ uint32_t lds_bound(const uint32_t* w, uint32_t lo,
                                              uint32_t hi, uint32_t key,
                                              bool upper) {
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    uint32_t v = w[mid];
    if (upper ? v <= key : v < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a hop's probe value: the seed's B component (src 0) or Z column (src 1).
// A mask, not `?:` on the two arrays — that becomes a selected address and
// sends the seed registers to scratch.
__device__ __forceinline__ uint32_t chain_key(int32_t src, uint32_t b,
                                              uint32_t z) {
  uint32_t take_b = src == 0 ? 0xFFFFFFFFu : 0u;
  return (b & take_b) | (z & ~take_b);
}

// first probe of a direct / table32 hop for all of a thread's seeds,
// issued back to back and not waited for: the hop kind is one
// block-uniform branch around the seed loop, and the direct table takes a
// clamped index (its range check is applied when the probe is finished)
__device__ __forceinline__ void chain_probe_issue(
    const ChainHops& hops, int h, const uint32_t (&sb)[kChainSeeds],
    const uint32_t (&sz)[kChainSeeds],
    uint32_t (&raw)[kChainSeeds]) {
  if (hops.direct[h] != nullptr) {
    // dense-value hop: counts[v - dmin], coalesced across the wave
#pragma unroll
    for (int u = 0; u < kChainSeeds; ++u) {
      uint64_t off = static_cast<uint64_t>(
          static_cast<int64_t>(chain_key(hops.src[h], sb[u], sz[u]))
          - hops.dmin[h]);
      bool ok = off < static_cast<uint64_t>(hops.dlen[h]);
      raw[u] = hops.direct[h][ok ? off : 0];
    }
    return;
  }
  // packed count-table hop: one 4-byte L2 load per seed
  uint32_t mask = static_cast<uint32_t>(hops.tmask[h]);
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u)
    raw[u] = hops.table32[h][
        h32(chain_key(hops.src[h], sb[u], sz[u])) & mask];
}

// multiply the hop's counts into prod; only a hash collision loads again
__device__ __forceinline__ void chain_probe_finish(
    const ChainHops& hops, int h, const uint32_t (&sb)[kChainSeeds],
    const uint32_t (&sz)[kChainSeeds],
    const uint32_t (&raw)[kChainSeeds],
    unsigned long long (&prod)[kChainSeeds]) {
  if (hops.direct[h] != nullptr) {
#pragma unroll
    for (int u = 0; u < kChainSeeds; ++u) {
      uint64_t off = static_cast<uint64_t>(
          static_cast<int64_t>(chain_key(hops.src[h], sb[u], sz[u]))
          - hops.dmin[h]);
      prod[u] *= off < static_cast<uint64_t>(hops.dlen[h]) ? raw[u] : 0u;
    }
    return;
  }
  uint32_t mask = static_cast<uint32_t>(hops.tmask[h]);
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u) {
    uint32_t v = chain_key(hops.src[h], sb[u], sz[u]);
    uint32_t slot = h32(v) & mask;
    uint32_t e = raw[u];
    while (e != kTbl32Empty && (e >> 7) != v) {
      slot = (slot + 1) & mask;
      e = hops.table32[h][slot];
    }
    prod[u] *= e == kTbl32Empty ? 0u : (e & 0x7Fu);
  }
}

// u64 count-table hop: one 8-byte L2 load per seed (vs log2(n) lines),
// the four first probes issued together
__device__ __forceinline__ void chain_table64_hop(
    const ChainHops& hops, int h, const uint32_t (&sb)[kChainSeeds],
    const uint32_t (&sz)[kChainSeeds],
    unsigned long long (&prod)[kChainSeeds]) {
  uint32_t mask = static_cast<uint32_t>(hops.tmask[h]);
  unsigned long long raw[kChainSeeds];
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u)
    raw[u] = hops.table[h][
        h32(chain_key(hops.src[h], sb[u], sz[u])) & mask];
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u) {
    uint32_t v = chain_key(hops.src[h], sb[u], sz[u]);
    uint32_t slot = h32(v) & mask;
    unsigned long long e = raw[u];
    while (e != kTblEmpty && static_cast<uint32_t>(e >> 32) != v) {
      slot = (slot + 1) & mask;
      e = hops.table[h][slot];
    }
    prod[u] *= e == kTblEmpty ? 0ull : (e & 0xFFFFFFFFull);
  }
}

__device__ __forceinline__ bool chain_hop_is_probe32(const ChainHops& hops,
                                                     int h) {
  return hops.direct[h] != nullptr || hops.table32[h] != nullptr;
}

// seeds are monotone: one lower bound for the thread's first seed, then
// every seed of the thread is matched in registers against the 8 window
// keys read from the 16-byte boundary below that bound.  All keys left of
// a0 are < b[0] <= b[u], so a seed's matches start at a0 or later; when
// the last key read is above the seed they also end before it, and the
// count is the number of equal keys (pad keys are above such a seed).
// Otherwise the run may go on past the 8 keys: search.  (A seed past the
// end reads as 0 and counts nothing or garbage; its product is dropped.)
__device__ __forceinline__ void chain_merge_lds(
    const uint32_t* w, uint32_t n, const uint32_t (&b)[kChainSeeds],
    unsigned long long (&prod)[kChainSeeds]) {
  uint32_t lo0 = lds_lower_bound_fixed(w, n, b[0]);
  uint32_t a0 = lo0 & ~3u;
  uint4 w0 = *reinterpret_cast<const uint4*>(w + a0);
  uint4 w1 = *reinterpret_cast<const uint4*>(w + a0 + 4);
  uint32_t wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u) {
    uint32_t key = b[u], cnt = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) cnt += wv[i] == key;
    if (!(wv[7] > key)) {
      uint32_t lo = lds_bound(w, a0, n, key, false);
      cnt = lds_bound(w, lo, n, key, true) - lo;
    }
    prod[u] *= cnt;
  }
}

// window too large for LDS (or not above lds_min), or a src-1 hop: search
// global memory.  Off the hot path; region sizes are int64 by contract.
__device__ __forceinline__ void chain_global_hop(
    const int32_t* __restrict__ base, int64_t wspan, int32_t src,
    const uint32_t (&sb)[kChainSeeds],
    const uint32_t (&sz)[kChainSeeds],
    unsigned long long (&prod)[kChainSeeds]) {
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u) {
    uint32_t key = chain_key(src, sb[u], sz[u]);
    int64_t lo = lower_bound_u32(base, wspan, key);
    // match runs are tiny (one object per subject in typical star data):
    // walk forward a few cache-hot slots instead of paying a second full
    // log2(wspan) dependent-load chain
    int64_t hi = lo;
    while (hi < wspan && hi - lo < 4
           && static_cast<uint32_t>(base[hi]) == key) ++hi;
    if (hi - lo == 4 && hi < wspan
        && static_cast<uint32_t>(base[hi]) == key)
      hi = lo + upper_bound_u32(base + lo, wspan - lo, key);
    prod[u] *= static_cast<unsigned long long>(hi - lo);
  }
}

// one src-0 search hop of one 256-seed group, answered from the wave's
// slice (filled by chain_fill_slice) or, in the global tier, from memory
__device__ __forceinline__ void chain_window_hop(
    const uint32_t* lds, int tier, const int32_t* __restrict__ base,
    const ChainWin& w, const uint32_t (&sb)[kChainSeeds],
    const uint32_t (&sz)[kChainSeeds],
    unsigned long long (&prod)[kChainSeeds]) {
  if (tier == kChainDirect)
    chain_hist_read(lds, sb, w.first, w.last, prod);
  else if (tier == kChainMerge)
    chain_merge_lds(lds, static_cast<uint32_t>(w.span), sb, prod);
  else
    chain_global_hop(base, w.span, 0, sb, sz, prod);
}

// every hop but the further src-0 window hops, for one 256-seed group,
// multiplied into prod; products of seeds past the end come back as 0.
// hp or ht < 0: no window hop here, no probe issued ahead.
__device__ __forceinline__ void chain_group(
    const uint32_t* lds, const ChainHops& hops, int hp, int ht, int tier,
    const int32_t* __restrict__ base, const ChainWin& w,
    const uint32_t (&sb)[kChainSeeds], const uint32_t (&sz)[kChainSeeds],
    const uint32_t (&raw)[kChainSeeds], int64_t t, int g, int64_t m,
    unsigned long long (&prod)[kChainSeeds]) {
  if (hp >= 0) chain_window_hop(lds, tier, base, w, sb, sz, prod);
  if (ht >= 0) chain_probe_finish(hops, ht, sb, sz, raw, prod);
  for (int h = 0; h < hops.k; ++h) {
    if (h == hp || h == ht) continue;
    if (hops.table[h] != nullptr) {
      chain_table64_hop(hops, h, sb, sz, prod);
    } else if (chain_hop_is_probe32(hops, h)) {
      uint32_t r2[kChainSeeds];
      chain_probe_issue(hops, h, sb, sz, r2);
      chain_probe_finish(hops, h, sb, sz, r2, prod);
    } else if (hops.src[h] != 0) {
      chain_global_hop(hops.key32[h], hops.n[h], hops.src[h], sb, sz, prod);
    }
  }
  int64_t i0 = t * kChainTile + (g * kChainWave + threadIdx.x) * kChainSeeds;
#pragma unroll
  for (int u = 0; u < kChainSeeds; ++u)
    prod[u] = i0 + u < m ? prod[u] : 0ull;
}

// One wave per workgroup and one tile at a time: the tile's loads go out
// back to back, its first table probe is issued before the LDS work and
// consumed after it, and what hides the memory latency is the other waves
// of the CU, each on a tile of its own.  There are no per-seed predicates:
// seeds past the end read as 0 and their products are dropped when the tile
// is summed.
__global__ void __launch_bounds__(kChainWave, 4)
chain_count_kernel(const int32_t* __restrict__ seed_b,
                   const int32_t* __restrict__ seed_z, int64_t m,
                   ChainHops hops, const int64_t* __restrict__ win,
                   unsigned long long* __restrict__ parts, int n_parts) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kChainSpan + kChainPad];
  unsigned long long acc = 0;
  // hp: the src-0 window hop whose rows are loaded with the tile's seeds;
  // ht: the table hop whose first probe is issued ahead of the window work;
  // more: there are further src-0 window hops, which reuse the slice once
  // hp has been consumed
  int hp = -1, ht = -1;
  bool more = false;
  for (int h = hops.k - 1; h >= 0; --h) {
    if (chain_hop_is_probe32(hops, h)) {
      ht = h;
    } else if (hops.table[h] == nullptr && hops.src[h] == 0) {
      more = hp >= 0;
      hp = h;
    }
  }
  // lean: no hop besides hp and ht
  const bool lean = hops.k == (hp >= 0) + (ht >= 0);
  const bool vec = ((reinterpret_cast<uintptr_t>(seed_b)
                     | reinterpret_cast<uintptr_t>(seed_z)) & 15) == 0;
  for (int64_t t = blockIdx.x; t * kChainTile < m; t += gridDim.x) {
    ChainTileIn cur;
    ChainWin w_cur = chain_load_win(win, t, hops.k, hp, 0, 0);
    chain_load_tile(cur, t, seed_b, seed_z, m, hops, hp, w_cur, vec);
    uint32_t raw[kChainGroups][kChainSeeds];
    if (ht >= 0 && !more) {
#pragma unroll
      for (int g = 0; g < kChainGroups; ++g)
        chain_probe_issue(hops, ht, cur.b[g], cur.z[g], raw[g]);
    }
    chain_tile_keys(cur, t, m, w_cur);
    int tier = kChainGlobal;
    const int32_t* base = nullptr;
    if (hp >= 0) {
      tier = chain_tier(w_cur, hops.lds_min);
      base = hops.key32[hp] + w_cur.lo;
      if (tier != kChainGlobal)
        chain_fill_slice(lds, tier, base, w_cur, cur.pw, true);
    }
    if (__builtin_expect(lean && (hp < 0 || tier == kChainDirect), 1)) {
      // the flagship's shape, fully unrolled: one bin read and one table
      // probe per seed
#pragma unroll
      for (int g = 0; g < kChainGroups; ++g) {
        unsigned long long prod[kChainSeeds];
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) prod[u] = 1;
        if (hp >= 0)
          chain_hist_read(lds, cur.b[g], w_cur.first, w_cur.last, prod);
        if (ht >= 0)
          chain_probe_finish(hops, ht, cur.b[g], cur.z[g], raw[g], prod);
        int64_t i0 = t * kChainTile
            + (g * kChainWave + threadIdx.x) * kChainSeeds;
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u)
          acc += i0 + u < m ? prod[u] : 0ull;
      }
    } else if (!more) {
      // every other chain and tier: one copy of the code, the group's
      // registers picked by index
#pragma unroll 1
      for (int g = 0; g < kChainGroups; ++g) {
        uint32_t sb[kChainSeeds], sz[kChainSeeds], rw[kChainSeeds];
        unsigned long long prod[kChainSeeds];
        chain_pick(cur.b, g, sb);
        chain_pick(cur.z, g, sz);
        chain_pick(raw, g, rw);
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) prod[u] = 1;
        chain_group(lds, hops, hp, ht, tier, base, w_cur, sb, sz, rw, t, g,
                    m, prod);
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) acc += prod[u];
      }
    } else {
      // further src-0 window hops reuse the slice once hp is consumed:
      // the window hops go first, one after the other, their counts kept
      // per seed, and every other hop follows (no probe was issued ahead:
      // the kept products have its registers)
      unsigned long long keep[kChainGroups][kChainSeeds];
#pragma unroll
      for (int g = 0; g < kChainGroups; ++g)
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) keep[g][u] = 1;
      for (int h = hp; h < hops.k; ++h) {
        if (h == ht || hops.table[h] != nullptr
            || chain_hop_is_probe32(hops, h) || hops.src[h] != 0)
          continue;
        ChainWin w = w_cur;
        int tier_h = tier;
        const int32_t* base_h = base;
        if (h != hp) {
          // this hop's rows did not come with the tile's loads
          w = chain_load_win(win, t, hops.k, h, w_cur.first, w_cur.last);
          tier_h = chain_tier(w, hops.lds_min);
          base_h = hops.key32[h] + w.lo;
          chain_wave_sync();  // the previous hop's reads are done
          if (tier_h != kChainGlobal)
            chain_fill_slice(lds, tier_h, base_h, w, cur.pw, false);
        }
#pragma unroll 1
        for (int g = 0; g < kChainGroups; ++g) {
          uint32_t sb[kChainSeeds], sz[kChainSeeds];
          unsigned long long prod[kChainSeeds];
          chain_pick(cur.b, g, sb);
          chain_pick(cur.z, g, sz);
          chain_pick(keep, g, prod);
          chain_window_hop(lds, tier_h, base_h, w, sb, sz, prod);
          chain_put(keep, g, prod);
        }
      }
#pragma unroll 1
      for (int g = 0; g < kChainGroups; ++g) {
        uint32_t sb[kChainSeeds], sz[kChainSeeds];
        unsigned long long prod[kChainSeeds];
        chain_pick(cur.b, g, sb);
        chain_pick(cur.z, g, sz);
        chain_pick(keep, g, prod);
        chain_group(lds, hops, -1, -1, kChainGlobal, nullptr, w_cur, sb, sz,
                    sb, t, g, m, prod);
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) acc += prod[u];
      }
    }
    chain_wave_sync();  // before the next tile refills the slice
  }
  // wave reduction then one device-scope atomic per wave (guide G12), on
  // one of n_parts partial sums: adds to ONE address are taken one after
  // the other, about 11 ns each as measured, which for the 4096 waves of a
  // full grid was half of the kernel
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off);
  if (threadIdx.x == 0 && acc)
    atomicAdd(parts + (blockIdx.x % n_parts) * kChainPartStride, acc);
}

// total = sum of the partial sums, which are left zeroed for the next query.
// With `host_out` (the device address of 16 host-mapped pinned bytes) the
// count goes straight to the host instead: count, a system-scope fence, then
// the flag the host spins on, so that no copy command follows the kernel.
__global__ void __launch_bounds__(kChainParts)
chain_total_kernel(unsigned long long* __restrict__ parts,
                   unsigned long long* __restrict__ total,
                   unsigned long long* __restrict__ host_out) {
  __shared__ unsigned long long wave_sum[kChainParts / 64];
  unsigned long long v = parts[threadIdx.x * kChainPartStride];
  parts[threadIdx.x * kChainPartStride] = 0;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x / 64] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int i = 0; i < kChainParts / 64; ++i) sum += wave_sum[i];
    if (host_out) {
      // one release fence between the two stores: the count has left the
      // device before the flag does
      __hip_atomic_store(host_out, sum, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(host_out + 1, 1ull, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      *total = sum;
    }
  }
}

// ---- packed tiles for the direct-count shape ------------------------------
// A registration whose every tile is counted directly (last - first <
// kChainSpan) needs 11 bits of a seed's key and of a window row's key once
// the tile's first key is known, so the serve path re-encodes its three
// streamed columns once, frame-of-reference per tile, 6 B per seed where
// the columns take 12:
//   seeds  one u32 per seed, (b - first_t) | ((z - zmin) << kPackKeyBits),
//          padded with zeros to whole tiles;
//   rows   one u16 per window row, key - first_t, each tile's rows padded to
//          a multiple of kPackChunk (16 bytes) with kPackPadRow, whose bin
//          lies behind the last one a seed can read;
//          (both permuted within the tile, see chain_pack_seed_at)
//   recs   per tile {first_t, the rows' offset and count in chunks,
//          last_t - first_t + 1}.
// The rule (chain_pack_rule_kernel and register_chain_serve):
//   the chain is exactly one src-0 search hop hp plus at most one direct or
//   table32 hop ht; every tile has last - first < kChainSpan and a window of
//   0 rows or more than lds_min; if ht reads z, max(z) - min(z) < 2^21; the
//   windows together hold at most 2 * (m + n_hp) rows (a key run that
//   straddles tiles repeats in each); a direct table ends below 2^32 and
//   neither table has more than 2^30 slots (byte offsets stay in 32 bits);
//   KOLIBRIE_CHAIN_PACKED is not 0.  Anything else keeps the columns.
constexpr int kPackKeyBits = 11;
constexpr int kPackZBits = 32 - kPackKeyBits;
constexpr int kPackChunk = 8;
constexpr int kDenseChunk = 16;  // key bytes per chunk of the dense format
constexpr uint32_t kPackPadRow = kChainSpan;
static_assert((1 << kPackKeyBits) == kChainSpan, "a key offset is 11 bits");
static_assert(kChainPad >= 1, "the pad rows' bin lies behind the slice");
// rows that travel with the tile's loads: two dwordx4 per lane
constexpr int kPackPreChunks = 2 * kChainWave;

enum ChainPackStat { kPackBad = 0, kPackRows = 1, kPackZMaxInv = 2,
                     kPackZMax = 3, kDenseBad = 4, kPackStats = 5 };

// the per-tile half of the rule, the tiles' row chunks (for the offsets)
// and the row total; with key_chunks, the tiles' key chunks of the dense
// format too
__global__ void chain_pack_rule_kernel(
    const int32_t* __restrict__ seed_b, int64_t m, int64_t n_tiles,
    const int64_t* __restrict__ win, int k, int hp, int lds_min,
    int64_t* __restrict__ chunks, int64_t* __restrict__ key_chunks,
    unsigned long long* __restrict__ stats) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n_tiles;
       t += (int64_t)gridDim.x * blockDim.x) {
    uint32_t first = static_cast<uint32_t>(seed_b[t * kChainTile]);
    uint32_t last =
        static_cast<uint32_t>(seed_b[min((t + 1) * kChainTile, m) - 1]);
    int64_t span = win[(t * k + hp) * 2 + 1] - win[(t * k + hp) * 2];
    bool ok = last - first < static_cast<uint32_t>(kChainSpan)
        && (span == 0 || span > lds_min);
    chunks[t] = (span + kPackChunk - 1) / kPackChunk;
    // the dense format's 16-byte chunks of one byte per key
    if (key_chunks)
      key_chunks[t] = ok ? (last - first) / kDenseChunk + 1 : 0;
    if (!ok) atomicOr(stats + kPackBad, 1ull);
    if (span)
      atomicAdd(stats + kPackRows, static_cast<unsigned long long>(span));
  }
}

// min and max of z as unsigned values (the min as the max of ~z, so that
// zeroed stats are the identity of both)
__global__ void chain_pack_zrange_kernel(
    const int32_t* __restrict__ seed_z, int64_t m,
    unsigned long long* __restrict__ stats) {
  uint32_t hi = 0, inv = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t z = static_cast<uint32_t>(seed_z[i]);
    hi = max(hi, z);
    inv = max(inv, ~z);
  }
  for (int off = 32; off > 0; off >>= 1) {
    hi = max(hi, static_cast<uint32_t>(__shfl_down(hi, off)));
    inv = max(inv, static_cast<uint32_t>(__shfl_down(inv, off)));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(stats + kPackZMax, static_cast<unsigned long long>(hi));
    atomicMax(stats + kPackZMaxInv, static_cast<unsigned long long>(inv));
  }
}

// Place i of a packed tile holds the tile's seed chain_pack_seed_at(i): a
// lane's dwordx4 takes every 64th seed of its group of 256, and likewise a
// lane's chunk takes every c-th row of the c <= 64 chunks loaded together.
// Sums do not mind the order, and the 64 lanes of one bin read or row add
// then go to neighbouring keys' bins, which lie in different LDS banks
// (consecutive seeds or rows in a lane put them 4 and 8 bins apart).
__host__ __device__ __forceinline__ int chain_pack_seed_at(int i) {
  return (i & ~255) | ((i & 3) << 6) | ((i >> 2) & 63);
}

// one block per tile (grid-stride): the tile's seeds, rows and record.
// `offs` is the inclusive prefix sum of the tiles' chunk counts.
__global__ void __launch_bounds__(kBlock)
chain_pack_tiles_kernel(const int32_t* __restrict__ seed_b,
                        const int32_t* __restrict__ seed_z, int64_t m,
                        int64_t n_tiles, const int32_t* __restrict__ key32,
                        const int64_t* __restrict__ win, int k, int hp,
                        const int64_t* __restrict__ offs, uint32_t zmin,
                        bool use_z, uint32_t* __restrict__ pseeds,
                        uint16_t* __restrict__ prows,
                        uint4* __restrict__ recs) {
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t first = static_cast<uint32_t>(seed_b[t * kChainTile]);
    uint32_t last =
        static_cast<uint32_t>(seed_b[min((t + 1) * kChainTile, m) - 1]);
    int64_t lo = win[(t * k + hp) * 2];
    int64_t span = win[(t * k + hp) * 2 + 1] - lo;
    int64_t chunks = (span + kPackChunk - 1) / kPackChunk;
    int64_t off = offs[t] - chunks;
    for (int i = threadIdx.x; i < kChainTile; i += kBlock) {
      int64_t idx = t * kChainTile + chain_pack_seed_at(i);
      uint32_t v = 0;
      if (idx < m) {
        v = static_cast<uint32_t>(seed_b[idx]) - first;
        if (use_z)
          v |= (static_cast<uint32_t>(seed_z[idx]) - zmin) << kPackKeyBits;
      }
      pseeds[t * kChainTile + i] = v;
    }
    uint16_t* rows = prows + off * kPackChunk;
    for (int64_t r = threadIdx.x; r < chunks * kPackChunk; r += kBlock) {
      // the block of up to kChainWave chunks this one is loaded with, and
      // the row it holds at this place
      int64_t blk = r / (kPackChunk * kChainWave);
      int64_t c = min<int64_t>(kChainWave, chunks - blk * kChainWave);
      int64_t in_blk = r % (kPackChunk * kChainWave);
      int64_t row = blk * (kPackChunk * kChainWave)
          + (in_blk % kPackChunk) * c + in_blk / kPackChunk;
      rows[r] = static_cast<uint16_t>(
          row < span ? static_cast<uint32_t>(key32[lo + row]) - first
                     : kPackPadRow);
    }
    if (threadIdx.x == 0)
      recs[t] = make_uint4(first, static_cast<uint32_t>(off),
                           static_cast<uint32_t>(chunks), last - first + 1);
  }
}

// the packed kernel's one further hop, with everything in 32 bits: the
// probed value is base + rel, where rel is the seed's key or z offset
enum ChainPackHt { kPackHtNone = 0, kPackHtDirect = 1, kPackHtTable32 = 2 };
struct ChainPackedHt {
  const uint32_t* tab;
  uint32_t kind, src;
  uint32_t zmin;
  uint32_t dmin, dlast;  // direct: slots [0, dlast] hold values dmin + slot
  uint32_t mask;         // table32
};

__device__ __forceinline__ uint32_t chain_pack_tab(const uint32_t* tab,
                                                   uint32_t slot) {
  // slot < 2^30: the byte offset stays a 32-bit register beside the base
  return *reinterpret_cast<const uint32_t*>(
      reinterpret_cast<const char*>(tab) + (slot << 2));
}

// one 8-row chunk into the bins: no index is checked, pad rows land in the
// bin behind the slice's last key
__device__ __forceinline__ void chain_pack_add(uint32_t* lds, const uint4& c) {
  uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    __hip_atomic_fetch_add(&lds[w[i] & 0xFFFFu], 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&lds[w[i] >> 16], 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// a seed's probe offset: its key bits (src 0) or its z bits (src 1), by a
// wave-uniform shift and width, so that the hop's source costs no branch
__device__ __forceinline__ uint32_t chain_pack_rel(uint32_t seed,
                                                   uint32_t shift,
                                                   uint32_t bits) {
  return __builtin_amdgcn_ubfe(seed, shift, bits);
}

// bin reads and the probe's finish for one tile.  `valid` seeds of the tile
// exist (the rest are padding, dropped by index in the tail tile).
template <int kKind, bool kTail>
__device__ __forceinline__ unsigned long long chain_packed_finish(
    const uint32_t* lds, const uint4 (&p)[kChainGroups],
    const uint32_t (&raw)[kChainGroups][kChainSeeds], const ChainPackedHt& ht,
    uint32_t base, uint32_t shift, uint32_t bits, uint32_t valid) {
  unsigned long long acc = 0;
#pragma unroll
  for (int g = 0; g < kChainGroups; ++g) {
    uint32_t s[kChainSeeds] = {p[g].x, p[g].y, p[g].z, p[g].w};
#pragma unroll
    for (int u = 0; u < kChainSeeds; ++u) {
      uint32_t cnt = lds[s[u] & (kChainSpan - 1)];
      uint32_t mul = 1;
      if (kKind == kPackHtDirect) {
        uint32_t off = chain_pack_rel(s[u], shift, bits) + (base - ht.dmin);
        mul = off <= ht.dlast ? raw[g][u] : 0u;
      } else if (kKind == kPackHtTable32) {
        uint32_t v = base + chain_pack_rel(s[u], shift, bits);
        uint32_t slot = h32(v) & ht.mask;
        uint32_t e = raw[g][u];
        while (e != kTbl32Empty && (e >> 7) != v) {
          slot = (slot + 1) & ht.mask;
          e = chain_pack_tab(ht.tab, slot);
        }
        mul = e == kTbl32Empty ? 0u : (e & 0x7Fu);
      }
      if (kTail) {
        uint32_t i = chain_pack_seed_at(
            (g * kChainWave + threadIdx.x) * kChainSeeds + u);
        mul = i < valid ? mul : 0u;
      }
      // the one product that can pass 32 bits
      acc += static_cast<unsigned long long>(cnt) * mul;
    }
  }
  return acc;
}

// a wave's tiles, for one kind of further hop
template <int kKind>
__device__ __forceinline__ unsigned long long chain_packed_tiles(
    uint32_t* lds, const uint4* __restrict__ pseeds,
    const uint4* __restrict__ prows, const uint4* __restrict__ recs,
    int64_t m, int64_t n_tiles, const ChainPackedHt& ht) {
  unsigned long long acc = 0;
  const uint32_t lane = threadIdx.x;
  const uint32_t pad2 = kPackPadRow * 0x10001u;
  const uint4 pad_chunk = make_uint4(pad2, pad2, pad2, pad2);
  const uint32_t shift = ht.src == 0 ? 0 : kPackKeyBits;
  const uint32_t bits = ht.src == 0 ? kPackKeyBits : kPackZBits;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint4 rec = recs[t];
    const uint32_t chunks = rec.z, nkeys = rec.w;
    const uint32_t base = ht.src == 0 ? rec.x : ht.zmin;
    // every load of the tile, back to back
    uint4 p[kChainGroups];
    const uint4* seeds = pseeds + t * (kChainTile / 4) + lane;
#pragma unroll
    for (int g = 0; g < kChainGroups; ++g) p[g] = seeds[g * kChainWave];
    const uint4* rows = prows + rec.y;
    uint4 rw[2] = {pad_chunk, pad_chunk};
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (lane + j * kChainWave < chunks) rw[j] = rows[lane + j * kChainWave];
    // the further hop's first probe, not waited for
    uint32_t raw[kChainGroups][kChainSeeds];
    if (kKind != kPackHtNone) {
#pragma unroll
      for (int g = 0; g < kChainGroups; ++g) {
        uint32_t s[kChainSeeds] = {p[g].x, p[g].y, p[g].z, p[g].w};
#pragma unroll
        for (int u = 0; u < kChainSeeds; ++u) {
          uint32_t rel = chain_pack_rel(s[u], shift, bits);
          if (kKind == kPackHtDirect) {
            uint32_t off = rel + (base - ht.dmin);
            raw[g][u] = chain_pack_tab(ht.tab, off <= ht.dlast ? off : 0u);
          } else {
            raw[g][u] = chain_pack_tab(ht.tab, h32(base + rel) & ht.mask);
          }
        }
      }
    }
    chain_hist_zero(lds, nkeys);
    chain_wave_sync();
    chain_pack_add(lds, rw[0]);
    chain_pack_add(lds, rw[1]);
    // a longer window is streamed
    for (uint32_t c = kPackPreChunks + lane; c < chunks; c += kChainWave)
      chain_pack_add(lds, rows[c]);
    chain_wave_sync();
    int64_t left = m - t * kChainTile;
    if (__builtin_expect(left >= kChainTile, 1))
      acc += chain_packed_finish<kKind, false>(lds, p, raw, ht, base, shift,
                                               bits, kChainTile);
    else
      acc += chain_packed_finish<kKind, true>(lds, p, raw, ht, base, shift,
                                              bits,
                                              static_cast<uint32_t>(left));
    chain_wave_sync();  // before the next tile refills the slice
  }
  return acc;
}

// The direct-count tier of chain_count_kernel over packed tiles: the same
// wave-owned 1024-seed tile, resident grid, 8 KB slice and partial sums,
// with 4 dwordx4 of seeds and 2 of rows per lane.
__global__ void __launch_bounds__(kChainWave, 4)
chain_count_packed_kernel(const uint4* __restrict__ pseeds,
                          const uint4* __restrict__ prows,
                          const uint4* __restrict__ recs, int64_t m,
                          int64_t n_tiles, ChainPackedHt ht,
                          unsigned long long* __restrict__ parts,
                          int n_parts) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kChainSpan + kChainPad];
  unsigned long long acc;
  if (ht.kind == kPackHtDirect)
    acc = chain_packed_tiles<kPackHtDirect>(lds, pseeds, prows, recs, m,
                                            n_tiles, ht);
  else if (ht.kind == kPackHtTable32)
    acc = chain_packed_tiles<kPackHtTable32>(lds, pseeds, prows, recs, m,
                                             n_tiles, ht);
  else
    acc = chain_packed_tiles<kPackHtNone>(lds, pseeds, prows, recs, m,
                                          n_tiles, ht);
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off);
  if (threadIdx.x == 0 && acc)
    atomicAdd(parts + (blockIdx.x % n_parts) * kChainPartStride, acc);
}

// ---- dense tiles (format 2): run lengths for the keys, bit-packed z --------
// Seeds and window rows are both sorted by key, so a tile's key column is
// its first key plus a run length per key, and z needs only the bits of its
// span.  Per tile t of kChainTile consecutive seeds with keys [first, last]:
//   keys   one byte per key of first..last: low nibble = this tile's seeds
//          with that key, high nibble = the window's rows with that key (the
//          full count, also for a key whose seeds straddle two tiles).
//          Padded with zero bytes to a multiple of kDenseChunk (16) bytes;
//          lane l reads chunk l, and chunk 64 + l when the tile has more
//          than 1024 keys.
//   zs     z - zmin of the tile's seeds at kW bits each, kW uniform for the
//          registration: lane l owns the seeds l, 64 + l, ... 960 + l of
//          the tile (slot s = seed / 64) as one string of 16 * kW bits,
//          slot s at bit s * kW, kept in kW / 2 dwords.  Of these the
//          first 4 * (kW / 8) are stored as planes of one dwordx4 per lane,
//          the rest as planes of one dword per lane (chain_dense_zs_at), so
//          that every load of the wave is one contiguous stretch.  The tail
//          tile is padded with zeros; a padding seed is never counted,
//          because no key's low nibble covers its place.
//   recs   per tile {first, the keys' offset in 16-byte chunks, the number
//          of keys, 0}.
// The kernel writes each seed's multiplicity from the further hop into LDS
// at its place in seed order, takes the wave's prefix sum of the lanes' seed
// nibbles, and then every lane walks its 16 keys: rows(key) times the
// multiplicities of the key's seeds.  No histogram: no bin zeroing and no
// LDS atomics.  Place p sits at dword p + p / 16 of the slice: when keys and
// seeds are 1:1 the lanes' reads are 16 places apart, and the odd stride of
// 17 dwords keeps them on different banks.
// The rule, on top of the packed format's: a further hop that reads z; no
// key with more than 15 of a tile's seeds; no key in a tile's range with more
// than 15 window rows; KOLIBRIE_CHAIN_DENSE is not 0.  Anything that misses
// only these keeps the 6-byte format.
constexpr int kDenseRound = kDenseChunk * kChainWave;  // keys per round
constexpr int kDenseMaxRun = 15;
constexpr int kDenseSlotStride = kChainWave + kChainWave / 16;
// places 0..1024 at dword p + p / 16: place 1024 (dword 1088) is what a
// key with no seed behind the tile's last seed reads, with its rows masked
// to 0 (chain_dense_keys), so the slice carries 16 spare dwords for it
constexpr int kDenseLds = kChainTile + kChainTile / 16 + 16;
// the widths the kernel is instantiated for; z spans below 2^21
constexpr int kDenseWidths[] = {8, 16, 18, 20, 22};
constexpr int kDenseNWidths = sizeof(kDenseWidths) / sizeof(kDenseWidths[0]);
static_assert(kDenseWidths[kDenseNWidths - 1] > kPackZBits,
              "every z span the packed rule admits is served");
static_assert(kChainSpan <= 2 * kDenseRound, "two rounds cover a tile's keys");

enum ChainDenseKind { kDenseDirect = 0, kDenseTable32 = 1 };

// the dword of a tile's zs that holds lane `lane`'s k-th dword
__host__ __device__ __forceinline__ int chain_dense_zs_at(int w, int lane,
                                                          int k) {
  int q4 = (w / 8) * 4;
  return k < q4 ? (k / 4) * (kChainWave * 4) + lane * 4 + (k & 3)
                : q4 * kChainWave + (k - q4) * kChainWave + lane;
}

// the per-element half of the dense rule: a run of 16 equal keys among one
// tile's seeds, or among the region's rows for a key inside some tile's
// range, sets stats[kDenseBad]
__global__ void chain_dense_rule_kernel(
    const int32_t* __restrict__ seed_b, int64_t m,
    const int32_t* __restrict__ key32, int64_t n,
    unsigned long long* __restrict__ stats) {
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       i < max(m, n); i += (int64_t)gridDim.x * blockDim.x) {
    if (i < m && (i % kChainTile) >= kDenseMaxRun
        && seed_b[i] == seed_b[i - kDenseMaxRun])
      bad = true;
    if (i < n && i >= kDenseMaxRun && key32[i] == key32[i - kDenseMaxRun]) {
      // in a tile's range unless it falls between two tiles or past the end
      uint32_t key = static_cast<uint32_t>(key32[i]);
      int64_t at = lower_bound_u32(seed_b, m, key);
      if (at < m && (at % kChainTile != 0
                     || static_cast<uint32_t>(seed_b[at]) == key))
        bad = true;
    }
  }
  if (bad) atomicOr(stats + kDenseBad, 1ull);
}

// one block per tile (grid-stride): nibble counts, z bits and the record,
// added into zeroed buffers.  `offs` is the inclusive prefix sum of the
// tiles' key chunks.
__global__ void __launch_bounds__(kBlock)
chain_dense_tiles_kernel(const int32_t* __restrict__ seed_b,
                         const int32_t* __restrict__ seed_z, int64_t m,
                         int64_t n_tiles, const int32_t* __restrict__ key32,
                         const int64_t* __restrict__ win, int k, int hp,
                         const int64_t* __restrict__ offs, uint32_t zmin,
                         int w, uint32_t* __restrict__ keys,
                         uint32_t* __restrict__ zs,
                         uint4* __restrict__ recs) {
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t first = static_cast<uint32_t>(seed_b[t * kChainTile]);
    uint32_t last =
        static_cast<uint32_t>(seed_b[min((t + 1) * kChainTile, m) - 1]);
    uint32_t nkeys = last - first + 1;
    int64_t chunks = (nkeys + kDenseChunk - 1) / kDenseChunk;
    int64_t off = offs[t] - chunks;
    uint32_t* tk = keys + off * (kDenseChunk / 4);
    uint32_t* tz = zs + t * (kChainTile / 32) * w;
    for (int i = threadIdx.x; i < kChainTile; i += kBlock) {
      int64_t idx = t * kChainTile + i;
      if (idx >= m) break;
      uint32_t kb = static_cast<uint32_t>(seed_b[idx]) - first;
      atomicAdd(tk + kb / 4, 1u << (8 * (kb & 3)));
      uint32_t rel = static_cast<uint32_t>(seed_z[idx]) - zmin;
      int lane = i & (kChainWave - 1), bit = (i / kChainWave) * w;
      int d = bit >> 5, sh = bit & 31;
      atomicOr(tz + chain_dense_zs_at(w, lane, d), rel << sh);
      if (sh + w > 32)
        atomicOr(tz + chain_dense_zs_at(w, lane, d + 1), rel >> (32 - sh));
    }
    int64_t lo = win[(t * k + hp) * 2];
    int64_t span = win[(t * k + hp) * 2 + 1] - lo;
    for (int64_t r = threadIdx.x; r < span; r += kBlock) {
      uint32_t kb = static_cast<uint32_t>(key32[lo + r]) - first;
      atomicAdd(tk + kb / 4, 0x10u << (8 * (kb & 3)));
    }
    if (threadIdx.x == 0)
      recs[t] = make_uint4(first, static_cast<uint32_t>(off), nkeys, 0u);
  }
}

// inclusive prefix sum over the wave's 64 lanes: within rows of 16 by DPP
// shifts, then across the rows by the two row broadcasts
__device__ __forceinline__ uint32_t chain_wave_scan(uint32_t x) {
  int v = static_cast<int>(x);
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // bcast:31
  return static_cast<uint32_t>(v);
}

// the seeds among a lane's 16 keys
__device__ __forceinline__ uint32_t chain_dense_seeds(const uint4& kc) {
  uint32_t s = (kc.x & 0x0F0F0F0Fu) + (kc.y & 0x0F0F0F0Fu)
      + (kc.z & 0x0F0F0F0Fu) + (kc.w & 0x0F0F0F0Fu);  // each byte <= 60
  return (s * 0x01010101u) >> 24;
}

__device__ __forceinline__ uint32_t chain_dense_mul_at(const uint32_t* lds,
                                                       uint32_t p) {
  return lds[p + (p >> 4)];
}

// a lane's 16 keys, whose seeds start at place `start`: rows(key) times the
// sum of its seeds' multiplicities.  The first seed of every key is read
// without a branch: a key with no seed reads a place it does not own, up to
// place 1024 in kDenseLds' spare dwords, which may never have been written,
// and its rows are masked to 0; only when some lane holds a key with two seeds or
// more does the wave go round again for the rest.
__device__ __forceinline__ unsigned long long chain_dense_keys(
    const uint32_t* lds, const uint4& kc, uint32_t start) {
  const uint32_t dw[4] = {kc.x, kc.y, kc.z, kc.w};
  unsigned long long acc = 0;
  uint32_t p = start;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t n4 = dw[j] & 0x0F0F0F0Fu;
    // 0xF0 in every byte whose seed nibble is not 0
    uint32_t bit = (n4 + 0x0F0F0F0Fu) & 0x10101010u;
    uint32_t rows4 = dw[j] & ((bit << 4) - bit);
    // byte b = the seeds of the dword's keys 0..b (at most 60), by shifts:
    // a 32-bit multiply runs at a quarter of their rate
    uint32_t upto = n4 + (n4 << 8);
    upto += upto << 16;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      uint32_t at =
          b == 0 ? p : p + __builtin_amdgcn_ubfe(upto, 8 * (b - 1), 8);
      uint32_t rows = __builtin_amdgcn_ubfe(rows4, 8 * b + 4, 4);
      acc += static_cast<unsigned long long>(rows)
          * chain_dense_mul_at(lds, at);
    }
    p += upto >> 24;
  }
  bool more = ((kc.x | kc.y | kc.z | kc.w) & 0x0E0E0E0Eu) != 0;
  if (__builtin_expect(__any(more), 0)) {
    // rare, so kept small: the 16 bytes shift through x
    uint32_t x = kc.x, y = kc.y, z = kc.z, w = kc.w;
    p = start;
#pragma unroll 1
    for (int k = 0; k < kDenseChunk; ++k) {
      uint32_t n = x & 15u, rows = (x >> 4) & 15u;
      unsigned long long sum = 0;
#pragma unroll 1
      for (uint32_t i = 1; i < n; ++i) sum += chain_dense_mul_at(lds, p + i);
      acc += rows * sum;
      p += n;
      x = (x >> 8) | (y << 24);
      y = (y >> 8) | (z << 24);
      z = (z >> 8) | (w << 24);
      w >>= 8;
    }
  }
  return acc;
}

// slot s of a lane's bit string
template <int kW>
__device__ __forceinline__ uint32_t chain_dense_rel(
    const uint32_t (&d)[kW / 2], int s) {
  const int bit = s * kW, k = bit >> 5, sh = bit & 31;
  if (sh + kW <= 32) return __builtin_amdgcn_ubfe(d[k], sh, kW);
  return __builtin_amdgcn_alignbit(d[k + 1 < kW / 2 ? k + 1 : k], d[k], sh)
      & ((1u << kW) - 1u);
}

template <int kW, int kKind>
__global__ void __launch_bounds__(kChainWave, 6)
chain_count_dense_kernel(const uint32_t* __restrict__ zs,
                         const uint4* __restrict__ keys,
                         const uint4* __restrict__ recs, int64_t n_tiles,
                         ChainPackedHt ht,
                         unsigned long long* __restrict__ parts,
                         int n_parts) {
  __shared__ uint32_t lds[kDenseLds];
  constexpr int kDw = kW / 2, kQuads = kDw / 4;
  constexpr int kSlots = kChainTile / kChainWave;
  const uint32_t lane = threadIdx.x;
  uint32_t* put = lds + lane + (lane >> 4);  // slot s goes to put[s * stride]
  const uint32_t zoff = ht.zmin - ht.dmin;   // direct: z offset -> table slot
  unsigned long long acc = 0;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint4 rec = recs[t];
    const uint32_t nkeys = rec.z;
    // every load of the tile, back to back
    const uint32_t* tz = zs + t * (kChainTile / 32 * kW);
    uint32_t d[kDw];
#pragma unroll
    for (int q = 0; q < kQuads; ++q) {
      uint4 v = reinterpret_cast<const uint4*>(tz)[q * kChainWave + lane];
      d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z;
      d[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 4 * kQuads; k < kDw; ++k)
      d[k] = tz[k * kChainWave + lane];
    const uint4* tk = keys + rec.y;
    uint4 kc0 = make_uint4(0, 0, 0, 0), kc1 = kc0;
    if (lane * kDenseChunk < nkeys) kc0 = tk[lane];
    if (kDenseRound + lane * kDenseChunk < nkeys) kc1 = tk[kChainWave + lane];
    // the further hop's first probe, not waited for
    uint32_t raw[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      uint32_t rel = chain_dense_rel<kW>(d, s);
      if (kKind == kDenseDirect) {
        uint32_t off = rel + zoff;
        raw[s] = chain_pack_tab(ht.tab, off <= ht.dlast ? off : 0u);
      } else {
        raw[s] = chain_pack_tab(ht.tab, h32(ht.zmin + rel) & ht.mask);
      }
    }
    // where each lane's keys' seeds start
    const uint32_t n0 = chain_dense_seeds(kc0);
    const uint32_t upto0 = chain_wave_scan(n0);
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      uint32_t mul = raw[s];
      if (kKind == kDenseDirect) {
        mul = chain_dense_rel<kW>(d, s) + zoff <= ht.dlast ? mul : 0u;
      } else if (kKind == kDenseTable32) {
        uint32_t v = ht.zmin + chain_dense_rel<kW>(d, s);
        uint32_t slot = h32(v) & ht.mask;
        uint32_t e = mul;
        while (e != kTbl32Empty && (e >> 7) != v) {
          slot = (slot + 1) & ht.mask;
          e = chain_pack_tab(ht.tab, slot);
        }
        mul = e == kTbl32Empty ? 0u : (e & 0x7Fu);
      }
      put[s * kDenseSlotStride] = mul;
    }
    chain_wave_sync();
    acc += chain_dense_keys(lds, kc0, upto0 - n0);
    if (nkeys > static_cast<uint32_t>(kDenseRound)) {
      const uint32_t n1 = chain_dense_seeds(kc1);
      const uint32_t base1 = __builtin_amdgcn_readlane(upto0, kChainWave - 1);
      acc += chain_dense_keys(lds, kc1, base1 + chain_wave_scan(n1) - n1);
    }
    chain_wave_sync();  // before the next tile's multiplicities
  }
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off);
  if (threadIdx.x == 0 && acc)
    atomicAdd(parts + (blockIdx.x % n_parts) * kChainPartStride, acc);
}

// KOLIBRIE_CHAIN_GRID caps the chain kernel's grid in place of the default
// below (0 or unset: the default), so that a small input can be made to
// walk several tiles per wave, and a large one to take a wave per tile.
inline int64_t chain_grid_cap() {
  const char* e = getenv("KOLIBRIE_CHAIN_GRID");
  return e ? std::max<int64_t>(0, atoll(e)) : 0;
}

// One wave per tile up to what the device keeps resident at once (asked of
// the runtime, since it follows the kernel's registers and LDS); the rest
// grid-stride.  All waves start together, so none queues behind a full
// first round.  A wave per tile measured the same (round 4).
template <class Kernel>
inline int chain_resident(Kernel kernel) {
  int per_cu = 0, dev = 0, cus = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, kernel, kChainWave, 0));
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(
      &cus, hipDeviceAttributeMultiprocessorCount, dev));
  return std::max(1, per_cu * cus);
}

inline int chain_grid(int64_t n_tiles, int64_t cap, bool packed = false) {
  static const int resident = chain_resident(chain_count_kernel);
  static const int resident_packed =
      chain_resident(chain_count_packed_kernel);
  int64_t grid = std::min<int64_t>(
      n_tiles, cap > 0 ? cap : packed ? resident_packed : resident);
  return static_cast<int>(std::max<int64_t>(1, grid));
}

// the chain kernel into `parts` (kChainParts zeroed partial sums) and their
// sum into *total; with parts == nullptr every wave adds to *total itself
// (a caller that brings no scratch), which must then be zero beforehand;
// with host_out the sum and a flag go to that host-mapped address instead
inline void chain_launch(const int32_t* seed_b, const int32_t* seed_z,
                         int64_t m, const ChainHops& hops,
                         const int64_t* win, unsigned long long* parts,
                         unsigned long long* total, int64_t n_tiles,
                         int64_t grid_cap, hipStream_t stream,
                         unsigned long long* host_out = nullptr) {
  hipLaunchKernelGGL(chain_count_kernel,
                     dim3(chain_grid(n_tiles, grid_cap)), dim3(kChainWave),
                     0, stream, seed_b, seed_z, m, hops, win,
                     parts ? parts : total, parts ? kChainParts : 1);
  HIP_OK(hipGetLastError());
  if (parts) {
    hipLaunchKernelGGL(chain_total_kernel, dim3(1), dim3(kChainParts), 0,
                       stream, parts, total, host_out);
    HIP_OK(hipGetLastError());
  }
}

// the dense kernel's instance for a width and a kind of further hop
using ChainDenseFn = void (*)(const uint32_t*, const uint4*, const uint4*,
                              int64_t, ChainPackedHt, unsigned long long*,
                              int);
template <int kW>
static ChainDenseFn chain_dense_fn_of(int kind) {
  return kind == kDenseDirect ? chain_count_dense_kernel<kW, kDenseDirect>
                              : chain_count_dense_kernel<kW, kDenseTable32>;
}
// one instance per entry of kDenseWidths, which is the only list of them
template <int kI = 0>
static ChainDenseFn chain_dense_fn(int w, int kind) {
  if constexpr (kI == kDenseNWidths) {
    TORCH_CHECK(false, "chain: no dense kernel for width ", w);
    return nullptr;
  } else {
    if (w == kDenseWidths[kI])
      return chain_dense_fn_of<kDenseWidths[kI]>(kind);
    return chain_dense_fn<kI + 1>(w, kind);
  }
}

// The hop lists of every chain entry point -> ChainHops.  All checks come
// before the first write: the struct's arrays hold kMaxHops entries.
static ChainHops chain_hops_from(const std::vector<at::Tensor>& hop_key32,
                                 const std::vector<int64_t>& hop_src,
                                 const std::vector<at::Tensor>& hop_table,
                                 const std::vector<int64_t>& hop_dmin) {
  const size_t k = hop_key32.size();
  TORCH_CHECK(k <= static_cast<size_t>(kMaxHops), "chain: at most ",
              kMaxHops, " hops, got ", k);
  TORCH_CHECK(hop_src.size() == k && hop_table.size() == k,
              "chain: hop_key32, hop_src and hop_table differ in length");
  TORCH_CHECK(hop_dmin.size() <= k, "chain: hop_dmin longer than the hops");
  auto is_direct = [&](size_t h) {
    return h < hop_dmin.size() && hop_dmin[h] >= 0;
  };
  for (size_t h = 0; h < k; ++h) {
    TORCH_CHECK(hop_key32[h].is_cuda() && hop_key32[h].dtype() == at::kInt,
                "chain: hop_key32 must be int32 on the device");
    if (hop_table[h].numel() == 0) continue;
    TORCH_CHECK(hop_table[h].is_cuda()
                && (hop_table[h].dtype() == at::kLong
                    || hop_table[h].dtype() == at::kInt),
                "chain: hop_table must be int32 or int64 on the device");
    TORCH_CHECK(!is_direct(h) || hop_table[h].dtype() == at::kInt,
                "chain: a direct-indexed hop_table must be int32");
  }
  ChainHops hops{};
  if (const char* e = getenv("KOLIBRIE_CHAIN_LDS_MIN"))
    hops.lds_min = atoi(e);
  hops.k = static_cast<int>(k);
  for (size_t h = 0; h < k; ++h) {
    hops.key32[h] = hop_key32[h].data_ptr<int32_t>();
    hops.n[h] = hop_key32[h].numel();
    hops.src[h] = static_cast<int32_t>(hop_src[h]);
    if (hop_table[h].numel() == 0) continue;
    if (is_direct(h)) {
      hops.direct[h] = reinterpret_cast<const uint32_t*>(
          hop_table[h].data_ptr<int32_t>());
      hops.dmin[h] = hop_dmin[h];
      hops.dlen[h] = hop_table[h].numel();
    } else if (hop_table[h].dtype() == at::kInt) {
      hops.table32[h] = reinterpret_cast<const uint32_t*>(
          hop_table[h].data_ptr<int32_t>());
    } else {
      hops.table[h] = reinterpret_cast<const unsigned long long*>(
          hop_table[h].data_ptr<int64_t>());
    }
    hops.tmask[h] = hop_table[h].numel() - 1;
  }
  return hops;
}

// per-tile hop windows into `win`; a non-null `zero` has its partial sums
// cleared by the same launch
inline void chain_bounds_launch(const int32_t* seed_b, int64_t m,
                                int64_t n_tiles, const ChainHops& hops,
                                int64_t* win, unsigned long long* zero,
                                hipStream_t stream) {
  hipLaunchKernelGGL(chain_tile_bounds, dim3(grid_for(n_tiles)), dim3(kBlock),
                     0, stream, seed_b, m, n_tiles, hops, win, zero);
  HIP_OK(hipGetLastError());
}

// Capture-friendly variant: caller owns the window + total buffers, no
// allocation and no device->host sync inside — the launch pair can be
// recorded into a hipGraph and replayed per query (launch-bound path).
void chain_count_into(at::Tensor seed_b, at::Tensor seed_z,
                      std::vector<at::Tensor> hop_key32,
                      std::vector<int64_t> hop_src,
                      std::vector<at::Tensor> hop_table,
                      std::vector<int64_t> hop_dmin,
                      at::Tensor win, at::Tensor total) {
  TORCH_CHECK(seed_b.is_cuda() && seed_b.dtype() == at::kInt
              && seed_z.is_cuda());
  TORCH_CHECK(win.dtype() == at::kLong && total.dtype() == at::kLong);
  int64_t m = seed_b.numel();
  ChainHops hops = chain_hops_from(hop_key32, hop_src, hop_table, hop_dmin);
  auto stream = cur_stream();
  total.zero_();
  if (m == 0) return;
  int64_t n_tiles = (m + kChainTile - 1) / kChainTile;
  TORCH_CHECK(win.numel() >= n_tiles * hops.k * 2, "win buffer too small");
  chain_bounds_launch(seed_b.data_ptr<int32_t>(), m, n_tiles, hops,
                      win.data_ptr<int64_t>(), nullptr, stream);
  // the caller brings no scratch for partial sums
  chain_launch(seed_b.data_ptr<int32_t>(), seed_z.data_ptr<int32_t>(), m,
               hops, win.data_ptr<int64_t>(), nullptr,
               reinterpret_cast<unsigned long long*>(
                   total.data_ptr<int64_t>()),
               n_tiles, chain_grid_cap(), stream);
}

// ---- C++ serving path (crush the per-query host
// floor).  All launch arguments for a cached COUNT chain live in a
// C++-side registry; one pybind call then does two direct kernel launches,
// the second of which stores the count and a flag into host-mapped pinned
// memory, and a spin on that flag — no Python plan walk, no torch
// dispatcher, no copy command, no graph replay floor (direct launches are
// ~3-4 µs each vs 10-16 µs replay, MI355X guide §graph-replay-floor).
struct ChainServe {
  at::Tensor seed_b, seed_z, win, total;
  // packed tiles (see chain_pack_tiles_kernel): they replace seed_b, seed_z
  // and win when the registration qualifies
  at::Tensor pseeds, prows, recs;
  // dense tiles (see chain_count_dense_kernel): they take the packed tiles'
  // place, with the same records tensor, when the dense rule holds too
  at::Tensor dkeys, dzs;
  int dense_w = 0, dense_kind = 0, dense_resident = 1;
  ChainPackedHt pht{};
  bool packed = false;  // either tile format
  bool dense = false;
  std::vector<at::Tensor> keep;
  ChainHops hops{};
  int64_t m = 0, n_tiles = 0, grid_cap = 0;
  // 16 host-mapped bytes, {count, flag}, and their device address
  int64_t* pinned = nullptr;
  unsigned long long* pinned_dev = nullptr;
  ~ChainServe() {
    if (pinned) (void)hipHostFree(pinned);
  }
};
static std::vector<std::unique_ptr<ChainServe>> g_chain_serves;

// Decide once whether the registration takes the packed tiles (the rule is
// stated at chain_pack_rule_kernel) and build them if so.  cs.win holds the
// windows already.  One host sync.
static void chain_try_pack(ChainServe& cs, const at::Tensor& seed_b,
                           const at::Tensor& seed_z,
                           const std::vector<at::Tensor>& hop_key32,
                           hipStream_t stream) {
  const char* env = getenv("KOLIBRIE_CHAIN_PACKED");
  if (env && atoi(env) == 0) return;
  const ChainHops& hops = cs.hops;
  int hp = -1, ht = -1;
  for (int h = 0; h < hops.k; ++h) {
    bool probe32 = hops.direct[h] != nullptr || hops.table32[h] != nullptr;
    if (probe32 && ht < 0) {
      ht = h;
    } else if (!probe32 && hops.table[h] == nullptr && hops.src[h] == 0
               && hp < 0) {
      hp = h;
    } else {
      return;  // a third hop, a u64 table, a src-1 search, a second of a kind
    }
  }
  if (hp < 0) return;
  ChainPackedHt pht{};
  bool use_z = false;
  if (ht >= 0) {
    pht.src = static_cast<uint32_t>(hops.src[ht]);
    use_z = hops.src[ht] != 0;
    constexpr int64_t kSlots = int64_t{1} << 30;
    if (hops.direct[ht] != nullptr) {
      if (hops.dlen[ht] > kSlots
          || hops.dmin[ht] + hops.dlen[ht] > (int64_t{1} << 32))
        return;
      pht.kind = kPackHtDirect;
      pht.tab = hops.direct[ht];
      pht.dmin = static_cast<uint32_t>(hops.dmin[ht]);
      pht.dlast = static_cast<uint32_t>(hops.dlen[ht] - 1);
    } else {
      if (hops.tmask[ht] >= kSlots) return;
      pht.kind = kPackHtTable32;
      pht.tab = hops.table32[ht];
      pht.mask = static_cast<uint32_t>(hops.tmask[ht]);
    }
  }
  // the dense format is tried when the further hop reads z
  const char* denv = getenv("KOLIBRIE_CHAIN_DENSE");
  const bool try_dense = use_z && !(denv && atoi(denv) == 0);
  auto opts = seed_b.options().dtype(at::kLong);
  auto stats = at::zeros({kPackStats}, opts);
  auto chunks = at::empty({try_dense ? 2 : 1, cs.n_tiles}, opts);
  auto* stats_u = reinterpret_cast<unsigned long long*>(
      stats.data_ptr<int64_t>());
  hipLaunchKernelGGL(chain_pack_rule_kernel, dim3(grid_for(cs.n_tiles)),
                     dim3(kBlock), 0, stream, seed_b.data_ptr<int32_t>(),
                     cs.m, cs.n_tiles, cs.win.data_ptr<int64_t>(), hops.k, hp,
                     hops.lds_min, chunks.data_ptr<int64_t>(),
                     try_dense ? chunks.data_ptr<int64_t>() + cs.n_tiles
                               : nullptr,
                     stats_u);
  HIP_OK(hipGetLastError());
  if (try_dense) {
    hipLaunchKernelGGL(chain_dense_rule_kernel,
                       dim3(grid_for(std::max(cs.m, hops.n[hp]))),
                       dim3(kBlock), 0, stream, seed_b.data_ptr<int32_t>(),
                       cs.m, hop_key32[hp].data_ptr<int32_t>(), hops.n[hp],
                       stats_u);
    HIP_OK(hipGetLastError());
  }
  if (use_z) {
    hipLaunchKernelGGL(chain_pack_zrange_kernel, dim3(grid_for(cs.m)),
                       dim3(kBlock), 0, stream, seed_z.data_ptr<int32_t>(),
                       cs.m, stats_u);
    HIP_OK(hipGetLastError());
  }
  auto offs = at::cumsum(chunks, 1);
  auto host = at::cat({stats, offs.select(1, cs.n_tiles - 1)}).cpu();
  const int64_t* st = host.data_ptr<int64_t>();
  const int64_t total_chunks = st[kPackStats];
  const uint32_t zmin = ~static_cast<uint32_t>(st[kPackZMaxInv]);
  const uint32_t zmax = static_cast<uint32_t>(st[kPackZMax]);
  if (st[kPackBad] != 0) return;
  if (use_z && zmax - zmin >= (1u << kPackZBits)) return;
  if (st[kPackRows] > 2 * (cs.m + hops.n[hp])) return;
  if (total_chunks > 0xFFFFFFFFll) return;
  pht.zmin = use_z ? zmin : 0u;
  cs.recs = at::empty({cs.n_tiles * 4}, seed_b.options().dtype(at::kInt));
  if (try_dense && st[kDenseBad] == 0
      && st[kPackStats + 1] <= 0xFFFFFFFFll) {
    // the narrowest instantiated width that holds zmax - zmin
    int w = 0;
    for (int i = kDenseNWidths - 1; i >= 0; --i)
      if (static_cast<uint64_t>(zmax - zmin) >> kDenseWidths[i] == 0)
        w = kDenseWidths[i];
    cs.dense_kind =
        pht.kind == kPackHtTable32 ? kDenseTable32 : kDenseDirect;
    // counts and bits are added into zeroed buffers
    cs.dkeys = at::zeros({st[kPackStats + 1] * (kDenseChunk / 4)},
                         seed_b.options().dtype(at::kInt));
    cs.dzs = at::zeros({cs.n_tiles * (kChainTile / 32) * w},
                       seed_b.options().dtype(at::kInt));
    hipLaunchKernelGGL(
        chain_dense_tiles_kernel,
        dim3(static_cast<int>(std::min<int64_t>(cs.n_tiles, 65536))),
        dim3(kBlock), 0, stream, seed_b.data_ptr<int32_t>(),
        seed_z.data_ptr<int32_t>(), cs.m, cs.n_tiles,
        hop_key32[hp].data_ptr<int32_t>(), cs.win.data_ptr<int64_t>(), hops.k,
        hp, offs.data_ptr<int64_t>() + cs.n_tiles, zmin, w,
        reinterpret_cast<uint32_t*>(cs.dkeys.data_ptr<int32_t>()),
        reinterpret_cast<uint32_t*>(cs.dzs.data_ptr<int32_t>()),
        reinterpret_cast<uint4*>(cs.recs.data_ptr<int32_t>()));
    HIP_OK(hipGetLastError());
    cs.dense_w = w;
    cs.dense_resident = chain_resident(chain_dense_fn(w, cs.dense_kind));
    cs.pht = pht;
    cs.packed = cs.dense = true;
    return;
  }
  cs.pseeds = at::empty({cs.n_tiles * kChainTile},
                        seed_b.options().dtype(at::kInt));
  cs.prows = at::empty({std::max<int64_t>(1, total_chunks) * kPackChunk},
                       seed_b.options().dtype(at::kShort));
  hipLaunchKernelGGL(
      chain_pack_tiles_kernel,
      dim3(static_cast<int>(std::min<int64_t>(cs.n_tiles, 65536))),
      dim3(kBlock), 0, stream, seed_b.data_ptr<int32_t>(),
      seed_z.data_ptr<int32_t>(), cs.m, cs.n_tiles,
      hop_key32[hp].data_ptr<int32_t>(), cs.win.data_ptr<int64_t>(), hops.k,
      hp, offs.data_ptr<int64_t>(), pht.zmin, use_z,
      reinterpret_cast<uint32_t*>(cs.pseeds.data_ptr<int32_t>()),
      reinterpret_cast<uint16_t*>(cs.prows.data_ptr<int16_t>()),
      reinterpret_cast<uint4*>(cs.recs.data_ptr<int32_t>()));
  HIP_OK(hipGetLastError());
  cs.pht = pht;
  cs.packed = true;
}

int64_t register_chain_serve(at::Tensor seed_b, at::Tensor seed_z,
                             std::vector<at::Tensor> hop_key32,
                             std::vector<int64_t> hop_src,
                             std::vector<at::Tensor> hop_table,
                             std::vector<int64_t> hop_dmin) {
  TORCH_CHECK(seed_b.is_cuda() && seed_b.dtype() == at::kInt
              && seed_z.is_cuda());
  auto cs = std::make_unique<ChainServe>();
  cs->hops = chain_hops_from(hop_key32, hop_src, hop_table, hop_dmin);
  cs->m = seed_b.numel();
  cs->grid_cap = chain_grid_cap();
  // the hops point into these tensors
  cs->keep = hop_key32;
  cs->keep.insert(cs->keep.end(), hop_table.begin(), hop_table.end());
  cs->n_tiles = (cs->m + kChainTile - 1) / kChainTile;
  cs->win = at::empty({std::max<int64_t>(1, cs->n_tiles * cs->hops.k * 2)},
                      seed_b.options().dtype(at::kLong));
  // total[0] = the count where no host address is given; behind it, from a
  // 128-byte boundary, the partial sums
  cs->total = at::zeros({kChainPartStride + kChainParts * kChainPartStride},
                        seed_b.options().dtype(at::kLong));
  // the count and the completion flag are stored by chain_total_kernel
  // itself: coherent host memory that the device addresses
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&cs->pinned), 16,
                       hipHostMallocMapped | hipHostMallocCoherent));
  HIP_OK(hipHostGetDevicePointer(reinterpret_cast<void**>(&cs->pinned_dev),
                                 cs->pinned, 0));
  cs->pinned[0] = cs->pinned[1] = 0;
  // the per-tile hop windows depend only on the CACHED seeds + hop
  // regions (immutable for this registration's lifetime: a store-version
  // bump re-registers), so compute them ONCE here instead of per query —
  // chain_tile_bounds was ~8% of the serve step.  It also zeroes the
  // accumulator, so the first serve call starts clean.
  if (cs->m > 0) {
    chain_bounds_launch(seed_b.data_ptr<int32_t>(), cs->m, cs->n_tiles,
                        cs->hops, cs->win.data_ptr<int64_t>(),
                        reinterpret_cast<unsigned long long*>(
                            cs->total.data_ptr<int64_t>()),
                        cur_stream());
    chain_try_pack(*cs, seed_b, seed_z, hop_key32, cur_stream());
  }
  if (cs->packed) {
    cs->win = at::Tensor();  // the records hold what the kernel needs of it
  } else {
    // the kernel reads each seed column with dwordx4 when its pointer is
    // 16-byte aligned; seed_z usually arrives as a slice of the PSO column,
    // aligned to 4 bytes only.  The seeds are immutable for this
    // registration's lifetime, so take an aligned copy once here.
    auto aligned16 = [](const at::Tensor& x) {
      bool ok = reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0;
      return ok ? x : x.clone();
    };
    cs->seed_b = aligned16(seed_b);
    cs->seed_z = aligned16(seed_z);
  }
  g_chain_serves.push_back(std::move(cs));
  return static_cast<int64_t>(g_chain_serves.size() - 1);
}

int64_t serve_chain_count(int64_t id) {
  auto& cs = *g_chain_serves.at(id);
  if (cs.m == 0) return 0;
  auto stream = cur_stream();
  int64_t* total_ptr = cs.total.data_ptr<int64_t>();
  volatile int64_t* flag = cs.pinned + 1;
  *flag = 0;
  // windows were precomputed at registration; the partial sums were zeroed
  // there (first call) or by chain_total_kernel in the previous call
  unsigned long long* total_u =
      reinterpret_cast<unsigned long long*>(total_ptr);
  if (cs.dense) {
    int64_t grid = std::min<int64_t>(
        cs.n_tiles, cs.grid_cap > 0 ? cs.grid_cap : cs.dense_resident);
    hipLaunchKernelGGL(
        chain_dense_fn(cs.dense_w, cs.dense_kind),
        dim3(static_cast<int>(grid)), dim3(kChainWave), 0, stream,
        reinterpret_cast<const uint32_t*>(cs.dzs.data_ptr<int32_t>()),
        reinterpret_cast<const uint4*>(cs.dkeys.data_ptr<int32_t>()),
        reinterpret_cast<const uint4*>(cs.recs.data_ptr<int32_t>()),
        cs.n_tiles, cs.pht, total_u + kChainPartStride, kChainParts);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(chain_total_kernel, dim3(1), dim3(kChainParts), 0,
                       stream, total_u + kChainPartStride, total_u,
                       cs.pinned_dev);
    HIP_OK(hipGetLastError());
  } else if (cs.packed) {
    hipLaunchKernelGGL(
        chain_count_packed_kernel,
        dim3(chain_grid(cs.n_tiles, cs.grid_cap, true)), dim3(kChainWave), 0,
        stream, reinterpret_cast<const uint4*>(cs.pseeds.data_ptr<int32_t>()),
        reinterpret_cast<const uint4*>(cs.prows.data_ptr<int16_t>()),
        reinterpret_cast<const uint4*>(cs.recs.data_ptr<int32_t>()), cs.m,
        cs.n_tiles, cs.pht, total_u + kChainPartStride, kChainParts);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(chain_total_kernel, dim3(1), dim3(kChainParts), 0,
                       stream, total_u + kChainPartStride, total_u,
                       cs.pinned_dev);
    HIP_OK(hipGetLastError());
  } else {
    chain_launch(cs.seed_b.data_ptr<int32_t>(),
                 cs.seed_z.data_ptr<int32_t>(), cs.m, cs.hops,
                 cs.win.data_ptr<int64_t>(), total_u + kChainPartStride,
                 total_u, cs.n_tiles, cs.grid_cap, stream, cs.pinned_dev);
  }
  // spin on the pinned flag, which chain_total_kernel stores after the
  // count: hipStreamSynchronize pays tens of µs of scheduler yield
  // latency.  Bounded: fall back to a real sync after ~2e9 spins (GPU
  // hung elsewhere).
  for (int64_t spins = 0; *flag == 0; ++spins) {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
    if (spins > 2000000000LL) {
      HIP_OK(hipStreamSynchronize(stream));
      break;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);  // the count is read after the flag
  return *static_cast<volatile int64_t*>(cs.pinned);
}

bool chain_serve_packed(int64_t id) {
  const auto& cs = g_chain_serves.at(id);
  TORCH_CHECK(cs != nullptr, "chain serve handle ", id, " was released");
  return cs->packed;
}

// 0: the columns, 1: the 6-byte packed tiles, 2: the dense tiles
int64_t chain_serve_format(int64_t id) {
  const auto& cs = g_chain_serves.at(id);
  TORCH_CHECK(cs != nullptr, "chain serve handle ", id, " was released");
  return cs->dense ? 2 : cs->packed ? 1 : 0;
}

// A dense registration's tiles decoded on the host, for the round-trip
// test: (seed_b, seed_z, the tiles' window row keys one tile after the
// other), ids as non-negative int64.
std::vector<at::Tensor> chain_serve_decode(int64_t id) {
  const auto& csp = g_chain_serves.at(id);
  TORCH_CHECK(csp != nullptr, "chain serve handle ", id, " was released");
  const ChainServe& cs = *csp;
  TORCH_CHECK(cs.dense, "chain_serve_decode: not a dense registration");
  auto keys_t = cs.dkeys.cpu(), zs_t = cs.dzs.cpu(), recs_t = cs.recs.cpu();
  const auto* keys = reinterpret_cast<const uint8_t*>(
      keys_t.data_ptr<int32_t>());
  const auto* zs = reinterpret_cast<const uint32_t*>(zs_t.data_ptr<int32_t>());
  const auto* recs = reinterpret_cast<const uint32_t*>(
      recs_t.data_ptr<int32_t>());
  const int w = cs.dense_w;
  std::vector<int64_t> sb, sz, rows;
  for (int64_t t = 0; t < cs.n_tiles; ++t) {
    const uint32_t first = recs[4 * t], nkeys = recs[4 * t + 2];
    const uint8_t* tk = keys + int64_t{recs[4 * t + 1]} * kDenseChunk;
    for (uint32_t j = 0; j < nkeys; ++j) {
      const int64_t key = int64_t{first} + j;
      for (int i = 0; i < (tk[j] & 15); ++i) sb.push_back(key);
      for (int i = 0; i < (tk[j] >> 4); ++i) rows.push_back(key);
    }
    const uint32_t* tz = zs + t * (kChainTile / 32) * w;
    const int64_t valid = std::min<int64_t>(kChainTile, cs.m - t * kChainTile);
    for (int i = 0; i < valid; ++i) {
      const int lane = i % kChainWave, bit = (i / kChainWave) * w;
      const int d = bit >> 5, sh = bit & 31;
      uint64_t v = tz[chain_dense_zs_at(w, lane, d)];
      if (sh + w > 32)
        v |= uint64_t{tz[chain_dense_zs_at(w, lane, d + 1)]} << 32;
      sz.push_back(int64_t{cs.pht.zmin}
                   + static_cast<int64_t>((v >> sh) & ((1u << w) - 1u)));
    }
  }
  auto out = [](const std::vector<int64_t>& v) {
    return at::tensor(v, at::kLong);
  };
  return {out(sb), out(sz), out(rows)};
}

void release_chain_serve(int64_t id) {
  if (id >= 0 && id < static_cast<int64_t>(g_chain_serves.size()))
    g_chain_serves[id].reset();
}

int64_t chain_count(at::Tensor seed_b, at::Tensor seed_z,
                    std::vector<at::Tensor> hop_key32,
                    std::vector<int64_t> hop_src,
                    std::vector<at::Tensor> hop_table,
                    std::vector<int64_t> hop_dmin) {
  TORCH_CHECK(seed_b.is_cuda() && seed_b.dtype() == at::kInt
              && seed_z.is_cuda());
  int64_t m = seed_b.numel();
  ChainHops hops = chain_hops_from(hop_key32, hop_src, hop_table, hop_dmin);
  auto total = at::zeros({1}, seed_b.options().dtype(at::kLong));
  if (m > 0) {
    auto stream = cur_stream();
    int64_t n_tiles = (m + kChainTile - 1) / kChainTile;
    auto win = at::empty({n_tiles * hops.k * 2},
                         seed_b.options().dtype(at::kLong));
    chain_bounds_launch(seed_b.data_ptr<int32_t>(), m, n_tiles, hops,
                        win.data_ptr<int64_t>(), nullptr, stream);
    auto parts = at::zeros({kChainParts * kChainPartStride},
                           seed_b.options().dtype(at::kLong));
    chain_launch(seed_b.data_ptr<int32_t>(), seed_z.data_ptr<int32_t>(), m,
                 hops, win.data_ptr<int64_t>(),
                 reinterpret_cast<unsigned long long*>(
                     parts.data_ptr<int64_t>()),
                 reinterpret_cast<unsigned long long*>(
                     total.data_ptr<int64_t>()),
                 n_tiles, chain_grid_cap(), stream);
  }
  return total.item<int64_t>();
}

// ------------------------------------------------------------ host launchers

// count phase of the K1 probes -> (lo, cnt) per probe row.  `sort_col`, when
// given, is the one varying probe column: from kProbeSortedMin probes up, if
// it ascends (and, with `need_nonneg`, starts non-negative: the low key half
// compares unsigned) the merge-path count runs instead of the plain one.
template <class Key>
static std::pair<at::Tensor, at::Tensor> count_phase(
    const at::Tensor& key12, Key key, int64_t m, const at::Tensor* sort_col,
    bool need_nonneg, hipStream_t stream) {
  auto n = key12.numel();
  auto lo = at::empty({m}, key12.options());
  auto cnt = at::empty({m}, key12.options().dtype(at::kInt));
  if (m == 0) return {lo, cnt};
  bool sorted = false;
  if (sort_col && m >= kProbeSortedMin) {
    // one cheap reduction decides the merge-path variant
    const auto& col = *sort_col;
    auto mono = at::all(col.slice(0, 1, m) >= col.slice(0, 0, m - 1));
    sorted = (need_nonneg ? mono & (col[0] >= 0) : mono).item<bool>();
  }
  if (sorted) {
    int64_t n_tiles = (m + kTile - 1) / kTile;
    auto wlo = at::empty({n_tiles}, key12.options());
    auto whi = at::empty({n_tiles}, key12.options());
    hipLaunchKernelGGL(probe_tile_bounds<Key>, dim3(grid_for(n_tiles)),
                       dim3(kBlock), 0, stream, key12.data_ptr<int64_t>(), n,
                       key, m, n_tiles, wlo.data_ptr<int64_t>(),
                       whi.data_ptr<int64_t>());
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL((probe_count<Key, true>), dim3(grid_for(m)),
                       dim3(kBlock), 0, stream, key12.data_ptr<int64_t>(), n,
                       key, m, wlo.data_ptr<int64_t>(),
                       whi.data_ptr<int64_t>(), lo.data_ptr<int64_t>(),
                       cnt.data_ptr<int32_t>());
  } else {
    hipLaunchKernelGGL((probe_count<Key, false>), dim3(grid_for(m)),
                       dim3(kBlock), 0, stream, key12.data_ptr<int64_t>(), n,
                       key, m, static_cast<const int64_t*>(nullptr),
                       static_cast<const int64_t*>(nullptr),
                       lo.data_ptr<int64_t>(), cnt.data_ptr<int32_t>());
  }
  HIP_OK(hipGetLastError());
  return {lo, cnt};
}

// emit phase of the K1 probes -> (li, b, z, carried...): per-probe-row emit
// for low fanout, output-parallel balanced emit for skewed ranges.  `carry`
// brings k and the input columns; the outputs are allocated here.  Without
// emit_b the b output stays empty.
static std::vector<at::Tensor> emit_phase(const at::Tensor& key12,
                                          const at::Tensor& z,
                                          const at::Tensor& lo,
                                          const at::Tensor& cnt, int64_t m,
                                          CarryCols carry, bool emit_b,
                                          hipStream_t stream) {
  auto opts_long = key12.options();
  auto opts_int = z.options();
  auto offs = at::cumsum(cnt, 0, at::kLong);
  int64_t total = m > 0 ? offs[-1].item<int64_t>() : 0;
  std::vector<at::Tensor> out = {at::empty({total}, opts_long),
                                 at::empty({emit_b ? total : 0}, opts_int),
                                 at::empty({total}, opts_int)};
  for (int j = 0; j < carry.k; ++j) {
    out.push_back(at::empty({total}, opts_int));
    carry.out[j] = out.back().data_ptr<int32_t>();
  }
  if (total == 0) return out;
  int64_t* li = out[0].data_ptr<int64_t>();
  int32_t* b = emit_b ? out[1].data_ptr<int32_t>() : nullptr;
  int32_t* zz = out[2].data_ptr<int32_t>();
  if (total >= 8 * m) {
    auto offs_full = at::zeros({m + 1}, opts_long);
    offs_full.narrow(0, 1, m).copy_(offs);
    hipLaunchKernelGGL(probe_emit_balanced, dim3(grid_for(total)),
                       dim3(kBlock), 0, stream, key12.data_ptr<int64_t>(),
                       z.data_ptr<int32_t>(), m, lo.data_ptr<int64_t>(),
                       offs_full.data_ptr<int64_t>(), total, carry, li, b, zz,
                       emit_b);
  } else {
    auto offs_excl = offs - cnt.to(at::kLong);
    hipLaunchKernelGGL(probe_emit, dim3(grid_for(m)), dim3(kBlock), 0, stream,
                       key12.data_ptr<int64_t>(), z.data_ptr<int32_t>(), m,
                       lo.data_ptr<int64_t>(), cnt.data_ptr<int32_t>(),
                       offs_excl.data_ptr<int64_t>(), carry, li, b, zz,
                       emit_b);
  }
  HIP_OK(hipGetLastError());
  return out;
}

static void check_exact_args(const at::Tensor& key12, const at::Tensor& keys) {
  TORCH_CHECK(key12.is_cuda() && keys.is_cuda(),
              "probe_exact: device tensors required");
  TORCH_CHECK(key12.dtype() == at::kLong && keys.dtype() == at::kLong);
}

static void check_range_args(const at::Tensor& key12, const at::Tensor& vals) {
  TORCH_CHECK(key12.is_cuda() && vals.is_cuda(),
              "probe_range: device tensors required");
  TORCH_CHECK(vals.dtype() == at::kInt);
}

// K1 probe — exact (packed 2-col key) mode.
std::vector<at::Tensor> probe_exact(at::Tensor key12, at::Tensor z,
                                    at::Tensor keys) {
  check_exact_args(key12, keys);
  TORCH_CHECK(z.is_cuda() && z.dtype() == at::kInt);
  auto m = keys.numel();
  auto stream = cur_stream();
  auto [lo, cnt] = count_phase(key12, ExactKey{keys.data_ptr<int64_t>()}, m,
                               &keys, false, stream);
  return emit_phase(key12, z, lo, cnt, m, CarryCols{}, true, stream);
}

// K1 probe — range (1-col prefix) mode.
std::vector<at::Tensor> probe_range(at::Tensor key12, at::Tensor z,
                                    at::Tensor vals) {
  check_range_args(key12, vals);
  TORCH_CHECK(z.is_cuda());
  auto m = vals.numel();
  auto stream = cur_stream();
  auto [lo, cnt] = count_phase(key12, RangeKey{vals.data_ptr<int32_t>()}, m,
                               nullptr, false, stream);
  return emit_phase(key12, z, lo, cnt, m, CarryCols{}, true, stream);
}

// K1 fused probe: inline key packing, optional merge-path for sorted keys,
// carry columns gathered during emit.  a/b: per-row column or constant.
std::vector<at::Tensor> probe_fused(at::Tensor key12, at::Tensor z,
                                    c10::optional<at::Tensor> a_col,
                                    int64_t a_const,
                                    c10::optional<at::Tensor> b_col,
                                    int64_t b_const,
                                    std::vector<at::Tensor> carry_cols,
                                    bool emit_b) {
  TORCH_CHECK(key12.is_cuda() && z.is_cuda());
  TORCH_CHECK(carry_cols.size() <= static_cast<size_t>(kMaxCarry));
  int64_t m = a_col.has_value() ? a_col->numel()
                                : (b_col.has_value() ? b_col->numel() : 0);
  TORCH_CHECK(m > 0, "probe_fused: need at least one probe column");
  CarryCols carry{};
  carry.k = static_cast<int>(carry_cols.size());
  for (size_t j = 0; j < carry_cols.size(); ++j) {
    TORCH_CHECK(carry_cols[j].is_cuda()
                && carry_cols[j].dtype() == at::kInt
                && carry_cols[j].numel() == m);
    carry.in[j] = carry_cols[j].data_ptr<int32_t>();
  }
  FusedKey key{a_col.has_value() ? a_col->data_ptr<int32_t>() : nullptr,
               a_const,
               b_col.has_value() ? b_col->data_ptr<int32_t>() : nullptr,
               b_const};
  // constant leading component: narrow every search to that contiguous
  // region ONCE (e.g. one predicate's slice) — the region usually stays
  // cache-resident, cutting the dependent-load chain per probe
  if (!key.a_col && key12.numel() > 0) {
    auto reg_keys = at::empty({2}, key12.options());
    reg_keys[0] = (a_const << 32);
    reg_keys[1] = (a_const << 32) | 0xFFFFFFFFLL;
    auto lo_t = at::searchsorted(key12, reg_keys[0], false, false);
    auto hi_t = at::searchsorted(key12, reg_keys[1], false, true);
    int64_t roff = lo_t.item<int64_t>();
    int64_t rend = hi_t.item<int64_t>();
    key12 = key12.narrow(0, roff, rend - roff);
    z = z.narrow(0, roff, rend - roff);
  }
  // merge-path when the single varying column is sorted (signed order is
  // the packed order when values share a sign; negatives skip the check)
  const at::Tensor* sort_col = nullptr;
  if ((key.a_col == nullptr) != (key.b_col == nullptr))
    sort_col = a_col.has_value() ? &*a_col : &*b_col;
  auto stream = cur_stream();
  auto [lo, cnt] = count_phase(key12, key, m, sort_col, b_col.has_value(),
                               stream);
  return emit_phase(key12, z, lo, cnt, m, carry, emit_b, stream);
}

// K1 count-only variants: COUNT(*) queries skip the emit pass entirely.
at::Tensor probe_exact_counts(at::Tensor key12, at::Tensor keys) {
  check_exact_args(key12, keys);
  return count_phase(key12, ExactKey{keys.data_ptr<int64_t>()}, keys.numel(),
                     nullptr, false, cur_stream()).second;
}

at::Tensor probe_range_counts(at::Tensor key12, at::Tensor vals) {
  check_range_args(key12, vals);
  return count_phase(key12, RangeKey{vals.data_ptr<int32_t>()}, vals.numel(),
                     nullptr, false, cur_stream()).second;
}

// The two sides of a K2 join, validated: int32 device columns, the same
// number (1..kMaxKeyCols) on each side.
struct HjSides {
  KeyCols probe, build;
  int64_t l, r;
};

static HjSides hj_sides(const std::vector<at::Tensor>& left_cols,
                        const std::vector<at::Tensor>& right_cols) {
  TORCH_CHECK(!left_cols.empty() && left_cols.size() == right_cols.size());
  TORCH_CHECK(left_cols.size() <= kMaxKeyCols, "hash_join: at most 4 key cols");
  HjSides s{};
  s.probe.k = s.build.k = static_cast<int>(left_cols.size());
  for (size_t j = 0; j < left_cols.size(); ++j) {
    TORCH_CHECK(left_cols[j].is_cuda() && right_cols[j].is_cuda());
    TORCH_CHECK(left_cols[j].dtype() == at::kInt && right_cols[j].dtype() == at::kInt);
    s.probe.c[j] = left_cols[j].data_ptr<int32_t>();
    s.build.c[j] = right_cols[j].data_ptr<int32_t>();
  }
  s.l = left_cols[0].numel();
  s.r = right_cols[0].numel();
  return s;
}

// The chained table over the build side.  Up to kHjLdsRows build rows each
// block stages its own in LDS, and this one stays empty.
struct HjTable {
  bool lds;
  at::Tensor heads, next;
  uint32_t mask = 0;
};

static HjTable hj_table(const HjSides& s, const at::TensorOptions& opts_int,
                        hipStream_t stream) {
  HjTable t{s.r <= kHjLdsRows, at::empty({0}, opts_int),
            at::empty({0}, opts_int)};
  if (t.lds) return t;
  // table size: next pow2 >= 2r
  uint64_t h = 1;
  while (h < static_cast<uint64_t>(2 * s.r)) h <<= 1;
  t.mask = static_cast<uint32_t>(h - 1);
  t.heads = at::full({static_cast<int64_t>(h)}, -1, opts_int);
  t.next = at::empty({s.r}, opts_int);
  hipLaunchKernelGGL(hj_build, dim3(grid_for(s.r)), dim3(kBlock), 0, stream,
                     s.build, s.r, t.mask, t.heads.data_ptr<int32_t>(),
                     t.next.data_ptr<int32_t>());
  HIP_OK(hipGetLastError());
  return t;
}

// per-probe-row match counts; both sides non-empty
static at::Tensor hj_counts(const HjSides& s, const HjTable& t,
                            const at::TensorOptions& opts_int,
                            hipStream_t stream) {
  auto cnt = at::empty({s.l}, opts_int);
  hipLaunchKernelGGL(t.lds ? hj_count<true> : hj_count<false>,
                     dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                     s.l, s.build, s.r, t.heads.data_ptr<int32_t>(),
                     t.next.data_ptr<int32_t>(), t.mask,
                     cnt.data_ptr<int32_t>());
  HIP_OK(hipGetLastError());
  return cnt;
}

// K2 hash join, count-only: per-probe-row match counts (no emit).
at::Tensor hash_join_counts(std::vector<at::Tensor> left_cols,
                            std::vector<at::Tensor> right_cols) {
  HjSides s = hj_sides(left_cols, right_cols);
  auto opts_int = left_cols[0].options();
  if (s.l == 0 || s.r == 0) return at::zeros({s.l}, opts_int);
  auto stream = cur_stream();
  return hj_counts(s, hj_table(s, opts_int, stream), opts_int, stream);
}

// K2 hash join: returns (li, ri) index pairs; multiset semantics.
std::vector<at::Tensor> hash_join(std::vector<at::Tensor> left_cols,
                                  std::vector<at::Tensor> right_cols) {
  HjSides s = hj_sides(left_cols, right_cols);
  auto opts_int = left_cols[0].options();
  auto opts_long = opts_int.dtype(at::kLong);
  if (s.l == 0 || s.r == 0) {
    return {at::empty({0}, opts_long), at::empty({0}, opts_long)};
  }
  auto stream = cur_stream();
  HjTable t = hj_table(s, opts_int, stream);
  auto cnt = hj_counts(s, t, opts_int, stream);
  auto offs = at::cumsum(cnt, 0, at::kLong);
  int64_t total = offs[-1].item<int64_t>();
  auto offs_excl = offs - cnt.to(at::kLong);
  auto li = at::empty({total}, opts_long);
  auto ri = at::empty({total}, opts_long);
  if (total > 0) {
    hipLaunchKernelGGL(t.lds ? hj_emit<true> : hj_emit<false>,
                       dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                       s.l, s.build, s.r, t.heads.data_ptr<int32_t>(),
                       t.next.data_ptr<int32_t>(), t.mask,
                       offs_excl.data_ptr<int64_t>(), li.data_ptr<int64_t>(),
                       ri.data_ptr<int64_t>());
    HIP_OK(hipGetLastError());
  }
  return {li, ri};
}

// K13 semi join: out[i] = (probe row i has an equal build row) ^ anti.
// The caller guarantees that no key cell is UNBOUND.  lds_tier: 1 takes the
// key set's LDS tier where the table fits it, anything else the table in
// global memory (the tier lost every measurement, see kSemiLdsSlots; the
// chained table of 3-4 columns ignores the knob).
at::Tensor semi_join_mask(std::vector<at::Tensor> probe_cols,
                          std::vector<at::Tensor> build_cols, bool anti,
                          int64_t lds_tier) {
  HjSides s = hj_sides(probe_cols, build_cols);
  for (size_t j = 0; j < probe_cols.size(); ++j) {
    TORCH_CHECK(probe_cols[j].dim() == 1 && build_cols[j].dim() == 1 &&
                    probe_cols[j].is_contiguous() &&
                    build_cols[j].is_contiguous(),
                "semi_join_mask: key columns must be contiguous 1-D");
    TORCH_CHECK(probe_cols[j].numel() == s.l && build_cols[j].numel() == s.r,
                "semi_join_mask: key columns of one side differ in length");
    TORCH_CHECK(probe_cols[j].device() == probe_cols[0].device() &&
                    build_cols[j].device() == probe_cols[0].device(),
                "semi_join_mask: key columns on different devices");
  }
  auto opts_int = probe_cols[0].options();
  auto opts_u8 = opts_int.dtype(at::kByte);
  const uint8_t flip = anti ? 1 : 0;
  if (s.l == 0) return at::empty({0}, opts_u8);
  if (s.r == 0) return at::full({s.l}, static_cast<int64_t>(flip), opts_u8);
  auto stream = cur_stream();
  auto out = at::empty({s.l}, opts_u8);
  if (s.probe.k > 2) {
    HjTable t = hj_table(s, opts_int, stream);
    hipLaunchKernelGGL(t.lds ? hj_exists<true> : hj_exists<false>,
                       dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                       s.l, s.build, s.r, t.heads.data_ptr<int32_t>(),
                       t.next.data_ptr<int32_t>(), t.mask, flip,
                       out.data_ptr<uint8_t>());
    HIP_OK(hipGetLastError());
    return out;
  }
  // key set: next power of two >= 2r slots, all EMPTY (-1 is ~0ull)
  int64_t slots = kSemiMinSlots;
  while (slots < 2 * s.r) slots <<= 1;
  TORCH_CHECK(slots <= (int64_t{1} << 32), "semi_join_mask: build side too large");
  const uint32_t mask = static_cast<uint32_t>(slots - 1);
  auto table = at::full({slots}, -1, opts_int.dtype(at::kLong));
  auto* tab = reinterpret_cast<unsigned long long*>(table.data_ptr<int64_t>());
  hipLaunchKernelGGL(semi_set_build, dim3(grid_for(s.r)), dim3(kBlock), 0,
                     stream, s.build, s.r, mask, tab);
  HIP_OK(hipGetLastError());
  const bool lds = lds_tier > 0 && slots <= kSemiLdsSlots;
  hipLaunchKernelGGL(lds ? semi_set_probe<true> : semi_set_probe<false>,
                     dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                     s.l, tab,
                     mask, flip, out.data_ptr<uint8_t>());
  HIP_OK(hipGetLastError());
  return out;
}

// K5 filter bytecode evaluation -> bool mask.
at::Tensor filter_bytecode(at::Tensor ops, at::Tensor args, at::Tensor consts,
                           std::vector<at::Tensor> cols, at::Tensor value_col,
                           int64_t n_rows) {
  TORCH_CHECK(cols.size() <= static_cast<size_t>(kMaxCols),
              "filter: at most 16 columns");
  auto out = at::empty({n_rows},
                       value_col.options().dtype(at::kBool));
  if (n_rows == 0) return out;
  // bytecode is tiny: keep it device-resident (caller moves it)
  TORCH_CHECK(ops.is_cuda() && args.is_cuda() && consts.is_cuda());
  FilterProg prog{};
  prog.ops = ops.data_ptr<int32_t>();
  prog.args = args.data_ptr<int32_t>();
  prog.consts = consts.data_ptr<double>();
  prog.n_ops = static_cast<int>(ops.numel());
  BindCols bc{};
  bc.k = static_cast<int>(cols.size());
  for (size_t j = 0; j < cols.size(); ++j) {
    TORCH_CHECK(cols[j].is_cuda() && cols[j].dtype() == at::kInt);
    bc.c[j] = cols[j].data_ptr<int32_t>();
  }
  hipLaunchKernelGGL(filter_eval, dim3(grid_for(n_rows)), dim3(kBlock), 0,
                     cur_stream(), prog, bc, value_col.data_ptr<double>(),
                     value_col.numel(), n_rows, out.data_ptr<bool>());
  HIP_OK(hipGetLastError());
  return out;
}

// The condition of a K14 join, validated.  `cond` is None (every key match
// survives) or (ops, args, consts, value_col, cols, sides): a K5 program
// whose column slot j is indexed by the left row where sides[j] == 0 and by
// the right row where it is 1.  The tensors stay referenced by the caller's
// tuple for the length of the call.
struct LjCond {
  FilterProg prog{};
  PairCols cols{};
  const double* value_col = nullptr;
  int64_t value_n = 0;
};

static LjCond lj_cond(const py::object& cond, const HjSides& s,
                      const at::Tensor& key0) {
  LjCond out;
  if (cond.is_none()) return out;
  auto t = cond.cast<py::tuple>();
  TORCH_CHECK(t.size() == 6, "left_join: cond is (ops, args, consts, "
                             "value_col, cols, sides)");
  auto ops = t[0].cast<at::Tensor>();
  auto args = t[1].cast<at::Tensor>();
  auto consts = t[2].cast<at::Tensor>();
  auto value_col = t[3].cast<at::Tensor>();
  auto cols = t[4].cast<std::vector<at::Tensor>>();
  auto sides = t[5].cast<std::vector<int64_t>>();
  TORCH_CHECK(ops.is_cuda() && args.is_cuda() && consts.is_cuda() &&
                  value_col.is_cuda(),
              "left_join: the program must be on the device");
  TORCH_CHECK(ops.device() == key0.device() &&
                  args.device() == key0.device() &&
                  consts.device() == key0.device() &&
                  value_col.device() == key0.device(),
              "left_join: program and keys on different devices");
  TORCH_CHECK(ops.dtype() == at::kInt && args.dtype() == at::kInt &&
                  consts.dtype() == at::kDouble &&
                  value_col.dtype() == at::kDouble,
              "left_join: program dtypes are int32, int32, float64, float64");
  TORCH_CHECK(ops.is_contiguous() && args.is_contiguous() &&
                  consts.is_contiguous() && value_col.is_contiguous() &&
                  ops.dim() == 1 && args.dim() == 1,
              "left_join: program tensors must be contiguous 1-D");
  TORCH_CHECK(ops.numel() == args.numel() && ops.numel() <= 128,
              "left_join: at most 128 ops, one arg each");
  TORCH_CHECK(cols.size() <= static_cast<size_t>(kMaxCols) &&
                  cols.size() == sides.size(),
              "left_join: at most 16 columns, one side flag each");
  for (size_t j = 0; j < cols.size(); ++j) {
    TORCH_CHECK(sides[j] == 0 || sides[j] == 1, "left_join: side is 0 or 1");
    TORCH_CHECK(cols[j].is_cuda() && cols[j].dtype() == at::kInt &&
                    cols[j].dim() == 1 && cols[j].is_contiguous() &&
                    cols[j].device() == key0.device(),
                "left_join: condition columns must be contiguous int32 on "
                "the keys' device");
    TORCH_CHECK(cols[j].numel() == (sides[j] ? s.r : s.l),
                "left_join: a condition column differs in length from its "
                "side");
    out.cols.c[j] = cols[j].data_ptr<int32_t>();
    if (sides[j]) out.cols.right_mask |= 1u << j;
  }
  out.prog.ops = ops.data_ptr<int32_t>();
  out.prog.args = args.data_ptr<int32_t>();
  out.prog.consts = consts.data_ptr<double>();
  out.prog.n_ops = static_cast<int>(ops.numel());
  out.value_col = value_col.data_ptr<double>();
  out.value_n = value_col.numel();
  return out;
}

static HjSides lj_sides(const std::vector<at::Tensor>& left_keys,
                        const std::vector<at::Tensor>& right_keys) {
  HjSides s = hj_sides(left_keys, right_keys);
  for (size_t j = 0; j < left_keys.size(); ++j) {
    TORCH_CHECK(left_keys[j].dim() == 1 && right_keys[j].dim() == 1 &&
                    left_keys[j].is_contiguous() &&
                    right_keys[j].is_contiguous(),
                "left_join: key columns must be contiguous 1-D");
    TORCH_CHECK(left_keys[j].numel() == s.l && right_keys[j].numel() == s.r,
                "left_join: key columns of one side differ in length");
    TORCH_CHECK(left_keys[j].device() == left_keys[0].device() &&
                    right_keys[j].device() == left_keys[0].device(),
                "left_join: key columns on different devices");
  }
  return s;
}

// survivors per left row (and the matched flags); both sides non-empty
static at::Tensor lj_counts(const HjSides& s, const HjTable& t,
                            const LjCond& c, uint8_t* matched,
                            const at::TensorOptions& opts_int,
                            hipStream_t stream) {
  auto cnt = at::empty({s.l}, opts_int);
  hipLaunchKernelGGL(t.lds ? lj_count<true> : lj_count<false>,
                     dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                     s.l, s.build, s.r, t.heads.data_ptr<int32_t>(),
                     t.next.data_ptr<int32_t>(), t.mask, c.prog, c.cols,
                     c.value_col, c.value_n, cnt.data_ptr<int32_t>(), matched);
  HIP_OK(hipGetLastError());
  return cnt;
}

// K14, count-only: int32[l] pairs of left row i that pass the condition.
at::Tensor left_join_counts(std::vector<at::Tensor> left_keys,
                            std::vector<at::Tensor> right_keys,
                            py::object cond) {
  HjSides s = lj_sides(left_keys, right_keys);
  auto opts_int = left_keys[0].options();
  LjCond c = lj_cond(cond, s, left_keys[0]);
  if (s.l == 0 || s.r == 0) return at::zeros({s.l}, opts_int);
  auto stream = cur_stream();
  return lj_counts(s, hj_table(s, opts_int, stream), c, nullptr, opts_int,
                   stream);
}

// K14 left join: (li int64[t], ri int64[t], matched uint8[l]).  The pairs
// are grouped by ascending li; the caller guarantees that no key cell is
// UNBOUND.
py::tuple left_join(std::vector<at::Tensor> left_keys,
                    std::vector<at::Tensor> right_keys, py::object cond) {
  HjSides s = lj_sides(left_keys, right_keys);
  auto opts_int = left_keys[0].options();
  auto opts_long = opts_int.dtype(at::kLong);
  auto opts_u8 = opts_int.dtype(at::kByte);
  LjCond c = lj_cond(cond, s, left_keys[0]);
  if (s.l == 0 || s.r == 0) {
    return py::make_tuple(at::empty({0}, opts_long), at::empty({0}, opts_long),
                          at::zeros({s.l}, opts_u8));
  }
  auto stream = cur_stream();
  HjTable t = hj_table(s, opts_int, stream);
  auto matched = at::empty({s.l}, opts_u8);
  auto cnt = lj_counts(s, t, c, matched.data_ptr<uint8_t>(), opts_int, stream);
  auto offs = at::cumsum(cnt, 0, at::kLong);
  int64_t total = offs[-1].item<int64_t>();
  auto offs_excl = offs - cnt.to(at::kLong);
  auto li = at::empty({total}, opts_long);
  auto ri = at::empty({total}, opts_long);
  if (total > 0) {
    hipLaunchKernelGGL(t.lds ? lj_emit<true> : lj_emit<false>,
                       dim3(grid_for(s.l)), dim3(kBlock), 0, stream, s.probe,
                       s.l, s.build, s.r, t.heads.data_ptr<int32_t>(),
                       t.next.data_ptr<int32_t>(), t.mask, c.prog, c.cols,
                       c.value_col, c.value_n, offs_excl.data_ptr<int64_t>(),
                       li.data_ptr<int64_t>(), ri.data_ptr<int64_t>());
    HIP_OK(hipGetLastError());
  }
  return py::make_tuple(li, ri, matched);
}

// K9 string predicate -> (uint8 mask of 0/1/2, int32[1] overflow count).
// `needle` is the pattern zero-padded to 256 bytes on the device, `m` its
// real length.  With fold != NONE the caller passes an ASCII needle already
// in the folded case.  The overflow count stays on the device (no sync); it
// is the number of rows the long-term kernel handled.
py::tuple str_match(at::Tensor ids, at::Tensor bytes, at::Tensor offsets,
                    int64_t V, at::Tensor needle, int64_t m, int64_t mode,
                    int64_t fold) {
  TORCH_CHECK(ids.is_cuda() && ids.dtype() == at::kInt && ids.dim() == 1
              && ids.is_contiguous(), "str_match: ids must be int32 on device");
  TORCH_CHECK(bytes.is_cuda() && bytes.dtype() == at::kByte
              && bytes.is_contiguous(), "str_match: bytes must be uint8");
  TORCH_CHECK(offsets.is_cuda() && offsets.dtype() == at::kLong
              && offsets.is_contiguous(), "str_match: offsets must be int64");
  TORCH_CHECK(needle.is_cuda() && needle.dtype() == at::kByte
              && needle.is_contiguous()
              && needle.numel() == kStrNeedleQ * 8,
              "str_match: needle must be 256 padded bytes on device");
  TORCH_CHECK(m >= 0 && m <= kStrMaxNeedle, "str_match: needle too long");
  TORCH_CHECK(mode >= SM_STARTS && mode <= SM_EQUALS, "str_match: bad mode");
  TORCH_CHECK(fold >= SF_NONE && fold <= SF_UPPER, "str_match: bad fold");
  TORCH_CHECK(V >= 0 && offsets.numel() >= V + 1,
              "str_match: offsets shorter than V + 1");
  const int64_t n = ids.numel();
  TORCH_CHECK(n < (int64_t(1) << 31), "str_match: too many rows");
  auto out = at::empty({n}, ids.options().dtype(at::kByte));
  auto ovf_count = at::zeros({1}, ids.options());
  if (n == 0) return py::make_tuple(out, ovf_count);
  // qword loads need an 8-aligned base (always true of a fresh allocation;
  // a view at an odd byte offset is refused rather than misread)
  const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(bp) % 8 == 0
              && reinterpret_cast<uintptr_t>(needle.data_ptr<uint8_t>()) % 8 == 0,
              "str_match: byte buffers must be 8-byte aligned");
  const bool may_overflow = (mode == SM_CONTAINS && m > 0);
  auto ovf_rows = at::empty({may_overflow ? n : 1}, ids.options());
  const uint64_t* nq =
      reinterpret_cast<const uint64_t*>(needle.data_ptr<uint8_t>());
  hipLaunchKernelGGL(str_match_rows, dim3(grid_for(n)), dim3(kBlock), 0,
                     cur_stream(), ids.data_ptr<int32_t>(), n, bp,
                     bytes.numel(), offsets.data_ptr<int64_t>(), V, nq,
                     static_cast<int>(m), static_cast<int32_t>(mode),
                     static_cast<int32_t>(fold), out.data_ptr<uint8_t>(),
                     ovf_count.data_ptr<int32_t>(),
                     ovf_rows.data_ptr<int32_t>());
  HIP_OK(hipGetLastError());
  if (may_overflow) {
    hipLaunchKernelGGL(str_match_long, dim3(kStrLongGrid), dim3(kBlock), 0,
                       cur_stream(), ids.data_ptr<int32_t>(), bp,
                       bytes.numel(), offsets.data_ptr<int64_t>(), nq,
                       static_cast<int>(m), static_cast<int32_t>(fold),
                       out.data_ptr<uint8_t>(),
                       ovf_count.data_ptr<int32_t>(),
                       ovf_rows.data_ptr<int32_t>());
    HIP_OK(hipGetLastError());
  }
  return py::make_tuple(out, ovf_count);
}

// K11 term_order wrappers.  Shared argument checks; returns the text base
// pointer (null for an empty blob, which no lane then reads: cap == 0).
static const uint8_t* term_order_check(const char* who, const at::Tensor& ids,
                                       const at::Tensor& bytes,
                                       const at::Tensor& offsets, int64_t V) {
  TORCH_CHECK(ids.is_cuda() && ids.dtype() == at::kInt && ids.dim() == 1
              && ids.is_contiguous(), who, ": ids must be int32 on device");
  TORCH_CHECK(bytes.is_cuda() && bytes.dtype() == at::kByte
              && bytes.dim() == 1 && bytes.is_contiguous(),
              who, ": bytes must be uint8");
  TORCH_CHECK(offsets.is_cuda() && offsets.dtype() == at::kLong
              && offsets.dim() == 1 && offsets.is_contiguous(),
              who, ": offsets must be int64");
  TORCH_CHECK(bytes.device() == ids.device()
              && offsets.device() == ids.device(),
              who, ": tensors on different devices");
  TORCH_CHECK(V >= 0 && offsets.numel() >= V + 1,
              who, ": offsets shorter than V + 1");
  const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(bp) % 8 == 0,
              who, ": text must be 8-byte aligned");
  return bp;
}

static void term_order_check_depth(const char* who, const at::Tensor& ids,
                                   const at::Tensor& depth) {
  TORCH_CHECK(depth.is_cuda() && depth.dtype() == at::kLong
              && depth.dim() == 1 && depth.is_contiguous()
              && depth.numel() == ids.numel()
              && depth.device() == ids.device(),
              who, ": depth must be int64[m] on the ids' device");
}

at::Tensor term_chunk_keys(at::Tensor ids, at::Tensor depth, at::Tensor bytes,
                           at::Tensor offsets, int64_t V) {
  const uint8_t* bp = term_order_check("term_chunk_keys", ids, bytes, offsets,
                                       V);
  term_order_check_depth("term_chunk_keys", ids, depth);
  const int64_t m = ids.numel();
  auto out = at::empty({m}, ids.options().dtype(at::kLong));
  if (m == 0) return out;
  hipLaunchKernelGGL(term_chunk_keys_kernel, dim3(grid_for(m)), dim3(kBlock),
                     0, cur_stream(), ids.data_ptr<int32_t>(),
                     depth.data_ptr<int64_t>(), m, bp, bytes.numel(),
                     offsets.data_ptr<int64_t>(), V, out.data_ptr<int64_t>());
  HIP_OK(hipGetLastError());
  return out;
}

at::Tensor term_adjacent_lcp(at::Tensor ids, at::Tensor depth,
                             at::Tensor same_group, at::Tensor bytes,
                             at::Tensor offsets, int64_t V) {
  const uint8_t* bp = term_order_check("term_adjacent_lcp", ids, bytes,
                                       offsets, V);
  term_order_check_depth("term_adjacent_lcp", ids, depth);
  TORCH_CHECK(same_group.is_cuda() && same_group.dtype() == at::kBool
              && same_group.dim() == 1 && same_group.is_contiguous()
              && same_group.numel() == ids.numel()
              && same_group.device() == ids.device(),
              "term_adjacent_lcp: same_group must be bool[m] on the ids' "
              "device");
  const int64_t m = ids.numel();
  auto out = at::empty({m}, ids.options().dtype(at::kLong));
  if (m == 0) return out;
  hipLaunchKernelGGL(term_adjacent_lcp_kernel, dim3(grid_for(m)),
                     dim3(kBlock), 0, cur_stream(), ids.data_ptr<int32_t>(),
                     depth.data_ptr<int64_t>(), same_group.data_ptr<bool>(),
                     m, bp, bytes.numel(), offsets.data_ptr<int64_t>(), V,
                     out.data_ptr<int64_t>());
  HIP_OK(hipGetLastError());
  return out;
}

at::Tensor term_numeric_class(at::Tensor ids, at::Tensor bytes,
                              at::Tensor offsets, int64_t V) {
  const uint8_t* bp = term_order_check("term_numeric_class", ids, bytes,
                                       offsets, V);
  const int64_t m = ids.numel();
  auto out = at::empty({m}, ids.options().dtype(at::kByte));
  if (m == 0) return out;
  hipLaunchKernelGGL(term_numeric_class_kernel, dim3(grid_for(m)),
                     dim3(kBlock), 0, cur_stream(), ids.data_ptr<int32_t>(),
                     m, bp, bytes.numel(), offsets.data_ptr<int64_t>(), V,
                     out.data_ptr<uint8_t>());
  HIP_OK(hipGetLastError());
  return out;
}

// K12 path_reach wrapper.  Every argument is checked on the host before the
// first launch: dtypes, device, contiguity, the CSR's shape and the value
// ranges of col and sources (one small read-back per call).
static void path_reach_check(const at::Tensor& row_ptr, const at::Tensor& col,
                             const at::Tensor& sources, int64_t max_hops,
                             int64_t levels_per_sync, int64_t hub_degree) {
  const char* who = "path_reach";
  TORCH_CHECK(row_ptr.is_cuda() && row_ptr.dtype() == at::kInt
              && row_ptr.dim() == 1 && row_ptr.is_contiguous(),
              who, ": row_ptr must be int32 on device");
  TORCH_CHECK(col.is_cuda() && col.dtype() == at::kInt && col.dim() == 1
              && col.is_contiguous(), who, ": col must be int32 on device");
  TORCH_CHECK(sources.is_cuda() && sources.dtype() == at::kInt
              && sources.dim() == 1 && sources.is_contiguous(),
              who, ": sources must be int32 on device");
  TORCH_CHECK(col.device() == row_ptr.device()
              && sources.device() == row_ptr.device(),
              who, ": tensors on different devices");
  TORCH_CHECK(row_ptr.numel() >= 1, who, ": row_ptr needs n_nodes + 1 entries");
  TORCH_CHECK(row_ptr.numel() - 1 <= INT32_MAX,
              who, ": more nodes than int32 node ids");
  TORCH_CHECK(col.numel() <= INT32_MAX,
              who, ": edge count does not fit the int32 row_ptr");
  TORCH_CHECK(sources.numel() <= INT32_MAX, who, ": too many sources");
  TORCH_CHECK(levels_per_sync >= 1 && levels_per_sync <= 1024,
              who, ": levels_per_sync must be in [1, 1024]");
  TORCH_CHECK(hub_degree >= 1, who, ": hub_degree must be >= 1");
  TORCH_CHECK(max_hops >= -1, who, ": max_hops must be >= 0, or -1 for none");
  const int64_t n_nodes = row_ptr.numel() - 1;
  // value ranges: [rp first, rp last, min rp step, col min, col max,
  //                src min, src max], neutral values for empty tensors
  auto l64 = row_ptr.options().dtype(at::kLong);
  auto scalar = [&](int64_t x) { return at::full({}, x, l64); };
  std::vector<at::Tensor> probe = {
      row_ptr[0].to(at::kLong), row_ptr[n_nodes].to(at::kLong),
      n_nodes ? at::diff(row_ptr).min().to(at::kLong) : scalar(0),
      col.numel() ? col.min().to(at::kLong) : scalar(0),
      col.numel() ? col.max().to(at::kLong) : scalar(-1),
      sources.numel() ? sources.min().to(at::kLong) : scalar(0),
      sources.numel() ? sources.max().to(at::kLong) : scalar(-1)};
  auto host = at::stack(probe).cpu();
  const int64_t* h = host.data_ptr<int64_t>();
  TORCH_CHECK(h[0] == 0 && h[1] == col.numel() && h[2] >= 0,
              who, ": row_ptr must rise from 0 to the edge count");
  TORCH_CHECK(h[3] >= 0 && h[4] < n_nodes, who, ": col value outside [0, n_nodes)");
  TORCH_CHECK(h[5] >= 0 && h[6] < n_nodes,
              who, ": source outside [0, n_nodes)");
}

// -> (source position int32[R], node int32[R], per-source reach counts
//     int64[S], per-source "reached itself" uint8[S], levels expanded).
// count_only leaves the two pair columns empty and never allocates them.
py::tuple path_reach(at::Tensor row_ptr, at::Tensor col, at::Tensor sources,
                     int64_t max_hops, int64_t levels_per_sync,
                     int64_t hub_degree, bool count_only) {
  path_reach_check(row_ptr, col, sources, max_hops, levels_per_sync,
                   hub_degree);
  const int64_t n_nodes = row_ptr.numel() - 1;
  const int64_t S = sources.numel();
  auto i32 = row_ptr.options();
  auto i64 = row_ptr.options().dtype(at::kLong);
  auto counts = at::zeros({S}, i64);
  auto self_hit = at::zeros({S}, row_ptr.options().dtype(at::kByte));
  std::vector<at::Tensor> pos_parts, node_parts;
  int64_t levels = 0;
  const int hub = static_cast<int>(std::min<int64_t>(hub_degree, INT32_MAX));
  if (S > 0 && n_nodes > 0 && max_hops != 0) {
    auto stream = cur_stream();
    // one allocation so one memset clears all three masks per pass
    auto masks = at::empty({3, n_nodes}, i64);
    auto queues = at::empty({2, std::max<int64_t>(n_nodes, kReachBatch)}, i32);
    auto state = at::empty({kReachStateWords}, i32);
    auto per_source = at::empty({kReachBatch}, i64);
    auto node_count = count_only ? at::Tensor() : at::empty({n_nodes}, i32);
    auto* mbase = reinterpret_cast<unsigned long long*>(
        masks.data_ptr<int64_t>());
    unsigned long long* seen = mbase;
    int32_t* qbase = queues.data_ptr<int32_t>();
    const int64_t qstride = queues.size(1);
    uint32_t* st = reinterpret_cast<uint32_t*>(state.data_ptr<int32_t>());
    const int32_t n32 = static_cast<int32_t>(n_nodes);
    // one fixed grid for the level and count kernels of every pass
    const int count_grid = static_cast<int>(std::min<int64_t>(
        kReachGrid, (n_nodes + kReachBlock - 1) / kReachBlock));
    bool drained = false;
    for (int64_t p0 = 0; p0 < S; p0 += kReachBatch) {
      const int n_src = static_cast<int>(std::min<int64_t>(kReachBatch, S - p0));
      const int32_t* src = sources.data_ptr<int32_t>() + p0;
      // a BFS that ran until its queue was empty leaves both frontier
      // masks zero: only `seen` (first in the allocation) needs clearing
      HIP_OK(hipMemsetAsync(mbase, 0,
                            sizeof(int64_t) * (drained ? 1 : 3) * n_nodes,
                            stream));
      drained = false;
      HIP_OK(hipMemsetAsync(st, 0, sizeof(int32_t) * kReachStateWords, stream));
      HIP_OK(hipMemsetAsync(per_source.data_ptr<int64_t>(), 0,
                            sizeof(int64_t) * kReachBatch, stream));
      unsigned long long* cur = mbase + n_nodes;
      unsigned long long* nxt = mbase + 2 * n_nodes;
      int32_t* q_in = qbase;
      int32_t* q_out = qbase + qstride;
      hipLaunchKernelGGL(path_reach_seed, dim3(1), dim3(kReachBatch), 0,
                         stream, src, n_src, n32, cur, q_in, st);
      HIP_OK(hipGetLastError());
      int slot = 0;
      int64_t done = 0;
      int32_t pass_levels = 0;
      while (max_hops < 0 || done < max_hops) {
        int64_t group = levels_per_sync;
        if (max_hops >= 0) group = std::min(group, max_hops - done);
        for (int64_t g = 0; g < group; ++g) {
          hipLaunchKernelGGL(path_reach_level, dim3(count_grid),
                             dim3(kReachBlock), 0, stream,
                             row_ptr.data_ptr<int32_t>(),
                             col.data_ptr<int32_t>(), n32, seen, cur, nxt,
                             q_in, q_out, st, slot, hub);
          HIP_OK(hipGetLastError());
          slot = (slot + 1) % 3;
          std::swap(cur, nxt);
          std::swap(q_in, q_out);
        }
        done += group;
        auto h = state.cpu();                    // the one sync per group
        const int32_t* hs = h.data_ptr<int32_t>();
        TORCH_CHECK(hs[4] == 0, "path_reach: work queue overflow");
        pass_levels = hs[3];
        drained = hs[slot] == 0;
        if (drained) break;
      }
      hipLaunchKernelGGL(path_reach_count, dim3(count_grid),
                         dim3(kReachBlock), 0, stream, seen, n32,
                         count_only ? nullptr : node_count.data_ptr<int32_t>(),
                         reinterpret_cast<unsigned long long*>(
                             per_source.data_ptr<int64_t>()));
      HIP_OK(hipGetLastError());
      hipLaunchKernelGGL(path_reach_self, dim3(1), dim3(kReachBatch), 0,
                         stream, src, n_src, n32, seen,
                         self_hit.data_ptr<uint8_t>() + p0);
      HIP_OK(hipGetLastError());
      counts.narrow(0, p0, n_src).copy_(per_source.narrow(0, 0, n_src));
      levels += pass_levels;
      if (count_only) continue;
      auto incl = at::cumsum(node_count, 0, at::kLong);
      const int64_t total = incl[n_nodes - 1].item<int64_t>();
      auto out_pos = at::empty({total}, i32);
      auto out_node = at::empty({total}, i32);
      if (total > 0) {
        hipLaunchKernelGGL(path_reach_emit, dim3(grid_for(n_nodes)),
                           dim3(kBlock), 0, stream, seen, n32,
                           incl.data_ptr<int64_t>(),
                           static_cast<int32_t>(p0), total,
                           out_pos.data_ptr<int32_t>(),
                           out_node.data_ptr<int32_t>());
        HIP_OK(hipGetLastError());
      }
      pos_parts.push_back(out_pos);
      node_parts.push_back(out_node);
    }
  }
  at::Tensor out_pos, out_node;
  if (pos_parts.empty()) {
    out_pos = at::empty({0}, i32);
    out_node = at::empty({0}, i32);
  } else if (pos_parts.size() == 1) {
    out_pos = pos_parts[0];
    out_node = node_parts[0];
  } else {
    out_pos = at::cat(pos_parts);
    out_node = at::cat(node_parts);
  }
  return py::make_tuple(out_pos, out_node, counts, self_hit, levels);
}

// ------------------------------------------------- host bulk N-Triples parse
// Native replacement for the reference's crossbeam parse pipeline
// (sparql_database.rs:636-795): one pass tokenizes lines, interns terms in
// a local dictionary and emits local-id triples; Python merges the (much
// smaller) unique-string table into the main dictionary and remaps the id
// columns vectorized.  RDF-star lines (`<<`) fall back to the Python path.
static inline std::string unescape_nt(const char* s, size_t len) {
  std::string out;
  out.reserve(len);
  for (size_t i = 0; i < len; ++i) {
    char c = s[i];
    if (c == '\\' && i + 1 < len) {
      char n = s[i + 1];
      switch (n) {
        case 'n': out.push_back('\n'); ++i; continue;
        case 't': out.push_back('\t'); ++i; continue;
        case 'r': out.push_back('\r'); ++i; continue;
        case '"': out.push_back('"'); ++i; continue;
        case '\\': out.push_back('\\'); ++i; continue;
        case 'u':
          if (i + 5 < len) {
            unsigned cp = std::stoul(std::string(s + i + 2, 4), nullptr, 16);
            // minimal UTF-8 encode
            if (cp < 0x80) out.push_back(static_cast<char>(cp));
            else if (cp < 0x800) {
              out.push_back(static_cast<char>(0xC0 | (cp >> 6)));
              out.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
            } else {
              out.push_back(static_cast<char>(0xE0 | (cp >> 12)));
              out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
              out.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
            }
            i += 5;
            continue;
          }
          break;
        default: break;
      }
    }
    out.push_back(c);
  }
  return out;
}

py::tuple parse_nlines_host(const std::string& text, bool quads) {
  std::unordered_map<std::string, int64_t> interned;
  std::vector<std::string> strings;
  std::vector<int64_t> ids;           // n*3 local ids
  std::vector<int64_t> fallback;      // line numbers for the Python path
  ids.reserve(1 << 16);

  auto intern = [&](std::string&& s) -> int64_t {
    auto it = interned.find(s);
    if (it != interned.end()) return it->second;
    int64_t id = static_cast<int64_t>(strings.size());
    interned.emplace(s, id);
    strings.push_back(std::move(s));
    return id;
  };

  size_t pos = 0, line_no = 0;
  const size_t n = text.size();
  while (pos < n) {
    size_t eol = text.find('\n', pos);
    if (eol == std::string::npos) eol = n;
    const char* line = text.data() + pos;
    size_t len = eol - pos;
    size_t save_pos = pos;
    pos = eol + 1;
    ++line_no;
    // trim
    size_t b = 0, e = len;
    while (b < e && isspace(static_cast<unsigned char>(line[b]))) ++b;
    while (e > b && isspace(static_cast<unsigned char>(line[e - 1]))) --e;
    if (b >= e || line[b] == '#') continue;
    // RDF-star or exotic: Python fallback
    bool star = false;
    for (size_t i = b; i + 1 < e; ++i)
      if (line[i] == '<' && line[i + 1] == '<') { star = true; break; }
    if (star) { fallback.push_back(static_cast<int64_t>(line_no - 1)); continue; }
    int64_t term_ids[4];
    const int max_terms = quads ? 4 : 3;
    int nt = 0;
    size_t i = b;
    bool ok = true;
    while (i < e && nt < max_terms) {
      while (i < e && isspace(static_cast<unsigned char>(line[i]))) ++i;
      if (i >= e) break;
      char c = line[i];
      if (c == '<') {
        size_t j = i + 1;
        while (j < e && line[j] != '>') ++j;
        if (j >= e) { ok = false; break; }
        term_ids[nt++] = intern(unescape_nt(line + i + 1, j - i - 1));
        i = j + 1;
      } else if (c == '"') {
        size_t j = i + 1;
        while (j < e && !(line[j] == '"' && line[j - 1] != '\\')) ++j;
        if (j >= e) { ok = false; break; }
        term_ids[nt++] = intern(unescape_nt(line + i + 1, j - i - 1));
        i = j + 1;
        // skip @lang / ^^<datatype>
        while (i < e && !isspace(static_cast<unsigned char>(line[i]))
               && line[i] != '.') {
          if (line[i] == '<') { while (i < e && line[i] != '>') ++i; }
          ++i;
        }
      } else if (c == '_' ) {
        size_t j = i;
        while (j < e && !isspace(static_cast<unsigned char>(line[j]))) ++j;
        term_ids[nt++] = intern(std::string(line + i, j - i));
        i = j;
      } else if (c == '.') {
        break;
      } else {
        ok = false;
        break;
      }
    }
    if (!ok || nt < 3 || (!quads && nt != 3)) {
      fallback.push_back(static_cast<int64_t>(line_no - 1));
      continue;
    }
    ids.push_back(term_ids[0]);
    ids.push_back(term_ids[1]);
    ids.push_back(term_ids[2]);
    if (quads) ids.push_back(nt == 4 ? term_ids[3] : -1);
    (void)save_pos;
  }
  const int64_t width = quads ? 4 : 3;
  auto t = at::from_blob(ids.data(),
                         {static_cast<int64_t>(ids.size()) / width, width},
                         at::kLong).clone();
  py::list pystrings;
  for (auto& s : strings) pystrings.append(py::bytes(s));
  py::list pyfallback;
  for (auto f : fallback) pyfallback.append(f);
  return py::make_tuple(t, pystrings, pyfallback);
}

// ---- multithreaded bulk parse (replaces the reference's crossbeam
// worker pipeline, sparql_database.rs:630-804 / :1264-1463): the input
// splits at line boundaries into one chunk per thread, each thread runs
// the single-pass tokenizer with a chunk-local intern table, then the
// main thread merges the (small) unique-string tables and the chunk
// threads remap their id columns in parallel.  The GIL is released for
// the whole native phase.
#include <deque>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

constexpr int kVocabShards = 32;

// open-addressing string_view -> id map (linear probing, stored 64-bit
// hash, power-of-two).  A node-based unordered_map pays one malloc plus
// a pointer chase per entry — at the 100M-triple bulk-load's ~43M unique
// terms (and ~130M chunk-local interns) that allocator traffic dominated
// the parse and merge phases.
struct FlatMap {
  struct Slot {
    const char* ptr = nullptr;   // nullptr => empty
    uint64_t hash = 0;
    int64_t id = 0;
    uint32_t len = 0;
  };
  std::vector<Slot> slots;
  size_t mask;
  size_t count = 0;
  FlatMap() : slots(1024), mask(1023) {}
  void grow() {
    std::vector<Slot> old = std::move(slots);
    size_t nsz = (mask + 1) * 2;
    slots.assign(nsz, Slot{});
    mask = nsz - 1;
    for (auto& s0 : old)
      if (s0.ptr) {
        size_t i = s0.hash & mask;
        while (slots[i].ptr) i = (i + 1) & mask;
        slots[i] = s0;
      }
  }
  // returns the slot index for key (h, sv); found=false means the slot
  // was claimed fresh — caller must fill ptr (e.g. repoint to an arena
  // copy) and id.  Grows BEFORE probing, so a returned index is valid
  // until the next find_or_insert.
  size_t find_or_insert(uint64_t h, std::string_view sv, bool& found) {
    if ((count + 1) * 10 >= (mask + 1) * 7) grow();
    size_t i = h & mask;
    for (;;) {
      Slot& sl = slots[i];
      if (sl.ptr == nullptr) {
        sl.ptr = sv.data();
        sl.hash = h;
        sl.len = static_cast<uint32_t>(sv.size());
        ++count;
        found = false;
        return i;
      }
      if (sl.hash == h && sl.len == sv.size()
          && memcmp(sl.ptr, sv.data(), sl.len) == 0) {
        found = true;
        return i;
      }
      i = (i + 1) & mask;
    }
  }
  // SIZE_MAX if absent
  size_t find(uint64_t h, std::string_view sv) const {
    size_t i = h & mask;
    for (;;) {
      const Slot& sl = slots[i];
      if (sl.ptr == nullptr) return SIZE_MAX;
      if (sl.hash == h && sl.len == sv.size()
          && memcmp(sl.ptr, sv.data(), sl.len) == 0) return i;
      i = (i + 1) & mask;
    }
  }
};

struct ParseChunkOut {
  // term views point into the shared input text (zero-copy for the
  // overwhelmingly common escape-free terms) or into `owned` (deque:
  // stable addresses) for unescaped materializations
  FlatMap interned;
  std::vector<std::string_view> views;
  std::vector<uint64_t> hashes;    // std::hash of each view, precomputed
  // view indices bucketed by hash % kVocabShards at parse time, so each
  // vocab-merge shard thread walks only its own items instead of
  // filter-scanning every chunk's full hash array
  std::vector<uint32_t> by_shard[kVocabShards];
  std::deque<std::string> owned;
  std::vector<int64_t> ids;
  std::vector<int64_t> fallback;   // chunk-local line numbers
  int64_t line_count = 0;
};

static void parse_chunk_nt(const char* data, size_t begin, size_t end,
                           bool quads, ParseChunkOut& out) {
  std::hash<std::string_view> sv_hasher;
  auto intern_sv = [&](std::string_view sv) -> int64_t {
    uint64_t hh = sv_hasher(sv);
    bool found;
    size_t si = out.interned.find_or_insert(hh, sv, found);
    if (found) return out.interned.slots[si].id;
    int64_t id = static_cast<int64_t>(out.views.size());
    out.interned.slots[si].id = id;
    out.views.push_back(sv);
    out.hashes.push_back(hh);
    out.by_shard[hh % kVocabShards].push_back(static_cast<uint32_t>(id));
    return id;
  };
  auto intern = [&](const char* ptr, size_t len) -> int64_t {
    if (memchr(ptr, '\\', len) == nullptr)
      return intern_sv(std::string_view(ptr, len));
    std::string u = unescape_nt(ptr, len);
    uint64_t hh = sv_hasher(std::string_view(u));
    bool found;
    size_t si = out.interned.find_or_insert(hh, std::string_view(u), found);
    if (found) return out.interned.slots[si].id;
    out.owned.push_back(std::move(u));
    std::string_view sv(out.owned.back());
    // the probe keyed on the TEMPORARY string — repoint to the stable copy
    out.interned.slots[si].ptr = sv.data();
    int64_t id = static_cast<int64_t>(out.views.size());
    out.interned.slots[si].id = id;
    out.views.push_back(sv);
    out.hashes.push_back(hh);
    out.by_shard[hh % kVocabShards].push_back(static_cast<uint32_t>(id));
    return id;
  };
  size_t pos = begin;
  int64_t line_no = 0;
  while (pos < end) {
    const char* nl = static_cast<const char*>(
        memchr(data + pos, '\n', end - pos));
    size_t eol = nl ? static_cast<size_t>(nl - data) : end;
    const char* line = data + pos;
    size_t len = eol - pos;
    pos = eol + 1;
    ++line_no;
    size_t b = 0, e = len;
    while (b < e && isspace(static_cast<unsigned char>(line[b]))) ++b;
    while (e > b && isspace(static_cast<unsigned char>(line[e - 1]))) --e;
    if (b >= e || line[b] == '#') continue;
    // RDF-star detection via memchr hops (the naive per-byte scan read
    // every line twice; memchr skips to the handful of '<' per line)
    bool star = false;
    for (const char* q = line + b;
         (q = static_cast<const char*>(
              memchr(q, '<', static_cast<size_t>(line + e - q)))) != nullptr;
         ++q) {
      if (q + 1 < line + e && q[1] == '<') { star = true; break; }
    }
    if (star) { out.fallback.push_back(line_no - 1); continue; }
    int64_t term_ids[4];
    const int max_terms = quads ? 4 : 3;
    int nt = 0;
    size_t i = b;
    bool ok = true;
    while (i < e && nt < max_terms) {
      while (i < e && isspace(static_cast<unsigned char>(line[i]))) ++i;
      if (i >= e) break;
      char c = line[i];
      if (c == '<') {
        const char* gt = static_cast<const char*>(
            memchr(line + i + 1, '>', e - i - 1));
        if (gt == nullptr) { ok = false; break; }
        size_t j = static_cast<size_t>(gt - line);
        term_ids[nt++] = intern(line + i + 1, j - i - 1);
        i = j + 1;
      } else if (c == '"') {
        size_t j = i + 1;
        for (;;) {
          const char* qq = static_cast<const char*>(
              memchr(line + j, '"', e - j));
          if (qq == nullptr) { j = e; break; }
          j = static_cast<size_t>(qq - line);
          if (line[j - 1] != '\\') break;
          ++j;
        }
        if (j >= e) { ok = false; break; }
        term_ids[nt++] = intern(line + i + 1, j - i - 1);
        i = j + 1;
        while (i < e && !isspace(static_cast<unsigned char>(line[i]))
               && line[i] != '.') {
          if (line[i] == '<') { while (i < e && line[i] != '>') ++i; }
          ++i;
        }
      } else if (c == '_') {
        size_t j = i;
        while (j < e && !isspace(static_cast<unsigned char>(line[j]))) ++j;
        term_ids[nt++] = intern_sv(std::string_view(line + i, j - i));
        i = j;
      } else if (c == '.') {
        break;
      } else {
        ok = false;
        break;
      }
    }
    if (!ok || nt < 3 || (!quads && nt != 3)) {
      out.fallback.push_back(line_no - 1);
      continue;
    }
    out.ids.push_back(term_ids[0]);
    out.ids.push_back(term_ids[1]);
    out.ids.push_back(term_ids[2]);
    if (quads) out.ids.push_back(nt == 4 ? term_ids[3] : -1);
  }
  out.line_count = line_no;
}

py::tuple parse_nlines_host_mt(const std::string& text, bool quads,
                               int64_t n_threads) {
  const size_t n = text.size();
  int nt = static_cast<int>(n_threads);
  if (nt <= 0) {
    nt = static_cast<int>(std::thread::hardware_concurrency());
    if (nt <= 0) nt = 8;
  }
  if (nt > 32) nt = 32;
  if (n < (1 << 20)) nt = 1;
  // chunk boundaries at line starts
  std::vector<size_t> starts(1, 0);
  for (int i = 1; i < nt; ++i) {
    size_t p = n * static_cast<size_t>(i) / nt;
    const char* nl = static_cast<const char*>(
        memchr(text.data() + p, '\n', n - p));
    starts.push_back(nl ? static_cast<size_t>(nl - text.data()) + 1 : n);
  }
  starts.push_back(n);
  std::vector<ParseChunkOut> outs(nt);
  std::vector<std::string> g_strings;
  std::vector<std::vector<int64_t>> remaps(nt);
  std::vector<int64_t> line_off(nt + 1, 0);
  int64_t total_rows = 0, total_fb = 0;
  {
    py::gil_scoped_release release;
    std::vector<std::thread> threads;
    for (int i = 0; i < nt; ++i)
      threads.emplace_back(parse_chunk_nt, text.data(), starts[i],
                           starts[i + 1], quads, std::ref(outs[i]));
    for (auto& t : threads) t.join();
    // merge unique-string tables (small relative to the line count)
    size_t uniq_upper0 = 0;
    for (int i = 0; i < nt; ++i) uniq_upper0 += outs[i].views.size();
    g_strings.reserve(uniq_upper0);
    std::unordered_map<std::string_view, int64_t> global;
    global.reserve(uniq_upper0 * 2);
    for (int i = 0; i < nt; ++i) {
      remaps[i].resize(outs[i].views.size());
      for (size_t k = 0; k < outs[i].views.size(); ++k) {
        auto it = global.find(outs[i].views[k]);
        if (it == global.end()) {
          int64_t id = static_cast<int64_t>(g_strings.size());
          g_strings.emplace_back(outs[i].views[k]);
          global.emplace(std::string_view(g_strings.back()), id);
          remaps[i][k] = id;
        } else {
          remaps[i][k] = it->second;
        }
      }
      line_off[i + 1] = line_off[i] + outs[i].line_count;
      total_rows += static_cast<int64_t>(outs[i].ids.size());
      total_fb += static_cast<int64_t>(outs[i].fallback.size());
    }
    // remap chunk-local ids to global ids, in parallel
    threads.clear();
    for (int i = 0; i < nt; ++i)
      threads.emplace_back([&, i]() {
        auto& rm = remaps[i];
        for (auto& v : outs[i].ids) v = rm[v];
      });
    for (auto& t : threads) t.join();
  }
  const int64_t width = quads ? 4 : 3;
  auto ids_t = at::empty({total_rows / width, width}, at::kLong);
  int64_t off = 0;
  int64_t* dst = ids_t.data_ptr<int64_t>();
  for (int i = 0; i < nt; ++i) {
    if (!outs[i].ids.empty()) {
      memcpy(dst + off, outs[i].ids.data(),
             outs[i].ids.size() * sizeof(int64_t));
      off += static_cast<int64_t>(outs[i].ids.size());
    }
  }
  py::list pystrings;
  for (auto& s : g_strings) pystrings.append(py::bytes(s));
  py::list pyfallback;
  for (int i = 0; i < nt; ++i)
    for (auto f : outs[i].fallback) pyfallback.append(f + line_off[i]);
  return py::make_tuple(ids_t, pystrings, pyfallback);
}

py::tuple parse_ntriples_host_mt(const std::string& text,
                                 int64_t n_threads) {
  return parse_nlines_host_mt(text, false, n_threads);
}

py::tuple parse_nquads_host_mt(const std::string& text, int64_t n_threads) {
  return parse_nlines_host_mt(text, true, n_threads);
}

// end-to-end file ingest: read + chunk-per-thread parse (GIL released),
// merge intern tables, then ONE GIL pass interns the UNIQUE strings
// straight into the Python Dictionary containers (str_to_id dict /
// id_to_str list / values list — no intermediate py::bytes round trip),
// and the id columns remap to global dictionary ids in parallel.
// Returns (int32 [n,3] global-id rows, fallback line numbers).
py::tuple parse_ntriples_file_encode(const std::string& path,
                                     int64_t n_threads,
                                     py::dict str_to_id, py::list id_to_str,
                                     py::list values, int64_t max_id) {
  const bool dbg = getenv("KOLIBRIE_PARSE_DEBUG") != nullptr;
  auto tick = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!dbg) return;
    auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[parse] %s: %.3fs\n", what,
            std::chrono::duration<double>(now - tick).count());
    tick = now;
  };
  std::string text;
  {
    py::gil_scoped_release release;
    FILE* f = fopen(path.c_str(), "rb");
    TORCH_CHECK(f != nullptr, "cannot open ", path);
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    text.resize(static_cast<size_t>(sz));
    size_t rd = fread(text.data(), 1, static_cast<size_t>(sz), f);
    fclose(f);
    TORCH_CHECK(rd == static_cast<size_t>(sz), "short read of ", path);
  }
  lap("read");
  const size_t n = text.size();
  int nt = static_cast<int>(n_threads);
  if (nt <= 0) {
    nt = static_cast<int>(std::thread::hardware_concurrency());
    if (nt <= 0) nt = 8;
  }
  if (nt > 32) nt = 32;
  if (n < (1 << 20)) nt = 1;
  std::vector<size_t> starts(1, 0);
  for (int i = 1; i < nt; ++i) {
    size_t p = n * static_cast<size_t>(i) / nt;
    const char* nl = static_cast<const char*>(
        memchr(text.data() + p, '\n', n - p));
    starts.push_back(nl ? static_cast<size_t>(nl - text.data()) + 1 : n);
  }
  starts.push_back(n);
  std::vector<ParseChunkOut> outs(nt);
  std::vector<std::vector<std::string_view>> shard_views;
  std::vector<std::vector<int64_t>> remaps(nt);
  std::vector<int64_t> line_off(nt + 1, 0);
  int64_t total_rows = 0;
  {
    py::gil_scoped_release release;
    std::vector<std::thread> threads;
    for (int i = 0; i < nt; ++i)
      threads.emplace_back(parse_chunk_nt, text.data(), starts[i],
                           starts[i + 1], false, std::ref(outs[i]));
    for (auto& t : threads) t.join();
    if (dbg) { py::gil_scoped_acquire a; lap("parallel parse"); }
    // SHARDED parallel merge: shard strings by hash; each thread owns one
    // shard, scans every chunk's view table and dedups only its shard
    // (remap entries encode (shard, local id); resolved after the GIL
    // interning pass assigns Python ids per shard)
    size_t uniq_upper = 0;
    for (int i = 0; i < nt; ++i) {
      remaps[i].resize(outs[i].views.size());
      uniq_upper += outs[i].views.size();
      line_off[i + 1] = line_off[i] + outs[i].line_count;
      total_rows += static_cast<int64_t>(outs[i].ids.size());
    }
    shard_views.resize(nt);
    {
      std::vector<std::thread> mthreads;
      for (int t = 0; t < nt; ++t)
        mthreads.emplace_back([&, t]() {
          std::unordered_map<std::string_view, int64_t> local;
          local.reserve(uniq_upper / std::max(1, nt) * 2 + 64);
          auto& sv = shard_views[t];
          for (int i = 0; i < nt; ++i) {
            auto& views = outs[i].views;
            auto& hs = outs[i].hashes;
            auto& rm = remaps[i];
            for (size_t k = 0; k < views.size(); ++k) {
              if (static_cast<int>(hs[k] % nt) != t) continue;
              auto it = local.find(views[k]);
              int64_t L;
              if (it == local.end()) {
                L = static_cast<int64_t>(sv.size());
                local.emplace(views[k], L);
                sv.push_back(views[k]);
              } else {
                L = it->second;
              }
              rm[k] = (static_cast<int64_t>(t) << 40) | L;
            }
          }
        });
      for (auto& t : mthreads) t.join();
    }
    if (dbg) { py::gil_scoped_acquire a; lap("merge"); }
  }
  // GIL pass: intern each shard's unique strings into the Python
  // dictionary (one SetDefault per string; a shared 0.0 float object for
  // the non-numeric majority)
  std::vector<std::vector<int64_t>> py_ids(shard_views.size());
  {
    PyObject* d = str_to_id.ptr();
    PyObject* lst = id_to_str.ptr();
    PyObject* vals = values.ptr();
    PyObject* zero = PyFloat_FromDouble(0.0);
    int64_t next_id = static_cast<int64_t>(PyList_GET_SIZE(lst));
    char numbuf[64];
    for (size_t t = 0; t < shard_views.size(); ++t) {
      auto& sv = shard_views[t];
      auto& pid = py_ids[t];
      pid.resize(sv.size());
      for (size_t k = 0; k < sv.size(); ++k) {
        std::string_view s = sv[k];
        PyObject* key = PyUnicode_DecodeUTF8(
            s.data(), static_cast<Py_ssize_t>(s.size()), "replace");
        TORCH_CHECK(key != nullptr, "utf-8 decode failed");
        TORCH_CHECK(next_id < max_id, "dictionary ID space exhausted");
        PyObject* idobj = PyLong_FromLongLong(next_id);
        PyObject* prev = PyDict_SetDefault(d, key, idobj);  // borrowed
        if (prev != idobj) {
          pid[k] = PyLong_AsLongLong(prev);
          Py_DECREF(idobj);
          Py_DECREF(key);
          continue;
        }
        PyList_Append(lst, key);
        // numeric value column: full-consume strtod, non-finite -> 0.0
        double v = 0.0;
        char c0 = s.empty() ? 0 : s[0];
        if (((c0 >= '0' && c0 <= '9') || c0 == '-' || c0 == '+'
             || c0 == '.' || c0 == ' ' || c0 == '\t'
             || c0 == 'i' || c0 == 'I' || c0 == 'n' || c0 == 'N')
            && s.size() < sizeof(numbuf)) {
          memcpy(numbuf, s.data(), s.size());
          numbuf[s.size()] = '\0';
          char* endp = nullptr;
          double parsed = strtod(numbuf, &endp);
          if (endp != numbuf && endp != nullptr) {
            while (*endp == ' ' || *endp == '\t') ++endp;
            if (*endp == '\0' && std::isfinite(parsed)) v = parsed;
          }
        }
        if (v == 0.0) {
          PyList_Append(vals, zero);
        } else {
          PyObject* vobj = PyFloat_FromDouble(v);
          PyList_Append(vals, vobj);
          Py_DECREF(vobj);
        }
        Py_DECREF(idobj);
        Py_DECREF(key);
        pid[k] = next_id++;
      }
    }
    Py_DECREF(zero);
  }
  lap("dict intern");
  auto ids_t = at::empty({total_rows / 3, 3}, at::kInt);
  {
    py::gil_scoped_release release;
    std::vector<std::thread> threads;
    std::vector<int64_t> offs(nt + 1, 0);
    for (int i = 0; i < nt; ++i)
      offs[i + 1] = offs[i] + static_cast<int64_t>(outs[i].ids.size());
    int32_t* dst = ids_t.data_ptr<int32_t>();
    for (int i = 0; i < nt; ++i)
      threads.emplace_back([&, i]() {
        auto& rm = remaps[i];
        int32_t* d = dst + offs[i];
        for (size_t k = 0; k < outs[i].ids.size(); ++k) {
          int64_t e = rm[outs[i].ids[k]];
          d[k] = static_cast<int32_t>(static_cast<uint32_t>(
              py_ids[e >> 40][e & ((1LL << 40) - 1)]));
        }
      });
    for (auto& t : threads) t.join();
  }
  lap("remap");
  py::list pyfallback;
  for (int i = 0; i < nt; ++i)
    for (auto f : outs[i].fallback) pyfallback.append(f + line_off[i]);
  return py::make_tuple(ids_t, pyfallback);
}

// ------------------------------------------------------------ vocab annex
// Native bulk-vocabulary store (the C++-primary dictionary tail): once a
// database bulk-loads, the Python dictionary's prefix [0, P0) freezes and
// EVERY later term id lives here — sharded string->id maps with stable
// deque arenas, a by-id pointer index, and the float64 value column.
// Python's Dictionary consults it on lookup/encode/decode misses; result
// decode uses the batch exporter so only requested ids materialize as
// Python strings.
// append-only bump arena: one memcpy per interned string instead of a
// per-string malloc (a deque<std::string> arena paid ~43M heap
// allocations on a 100M-triple load — the dominant merge cost)
struct BumpArena {
  std::vector<std::unique_ptr<char[]>> blocks;
  size_t used = 0, cap = 0;
  std::string_view add(std::string_view sv) {
    if (blocks.empty() || used + sv.size() > cap) {
      // blocks.empty() guard: a zero-length first insert (e.g. the empty
      // literal "") must still allocate before blocks.back()
      size_t bs = std::max<size_t>(size_t(1) << 24, sv.size());
      blocks.emplace_back(new char[bs]);
      used = 0;
      cap = bs;
    }
    char* dst = blocks.back().get() + used;
    memcpy(dst, sv.data(), sv.size());
    used += sv.size();
    return std::string_view(dst, sv.size());
  }
};

struct VocabShard {
  FlatMap map;
  BumpArena arena;
};

struct Vocab {
  int nshards = kVocabShards;
  std::vector<VocabShard> shards;
  std::vector<std::string_view> by_id;  // index = id - base
  std::vector<double> values;
  int64_t base = -1;
  Vocab() : shards(nshards) {}
};
static std::vector<std::unique_ptr<Vocab>> g_vocabs;

static double parse_value_full(std::string_view s) {
  char c0 = s.empty() ? 0 : s[0];
  if (!((c0 >= '0' && c0 <= '9') || c0 == '-' || c0 == '+' || c0 == '.'
        || c0 == ' ' || c0 == '\t' || c0 == 'i' || c0 == 'I'
        || c0 == 'n' || c0 == 'N'))
    return 0.0;
  if (s.size() >= 63) return 0.0;
  char buf[64];
  memcpy(buf, s.data(), s.size());
  buf[s.size()] = '\0';
  char* endp = nullptr;
  double parsed = strtod(buf, &endp);
  if (endp == buf || endp == nullptr) return 0.0;
  while (*endp == ' ' || *endp == '\t') ++endp;
  if (*endp != '\0' || !std::isfinite(parsed)) return 0.0;
  return parsed;
}

int64_t vocab_create(int64_t base_id) {
  auto v = std::make_unique<Vocab>();
  v->base = base_id;
  g_vocabs.push_back(std::move(v));
  return static_cast<int64_t>(g_vocabs.size() - 1);
}

// create seeded with the Python dictionary's frozen prefix: the bulk
// parser dedups against these ids too (without this a prefix string —
// including "" at id 0, or any term interned before the first bulk
// load — would get a DUPLICATE annex id and constant-term queries
// would miss the bulk-loaded rows)
int64_t vocab_create_seeded(py::list strings) {
  auto v = std::make_unique<Vocab>();
  v->base = static_cast<int64_t>(strings.size());
  std::hash<std::string_view> hasher;
  int64_t i = 0;
  for (auto h : strings) {
    std::string str = py::cast<std::string>(h);
    std::string_view key(str);
    uint64_t hh = hasher(key);
    auto& sh = v->shards[hh % v->nshards];
    bool found;
    size_t si = sh.map.find_or_insert(hh, key, found);
    if (!found) {
      std::string_view sv = sh.arena.add(key);
      sh.map.slots[si].ptr = sv.data();
      sh.map.slots[si].id = i;
    }
    ++i;
  }
  g_vocabs.push_back(std::move(v));
  return static_cast<int64_t>(g_vocabs.size() - 1);
}

int64_t vocab_len(int64_t h) {
  return static_cast<int64_t>(g_vocabs.at(h)->by_id.size());
}

int64_t vocab_lookup(int64_t h, const std::string& s) {
  Vocab& v = *g_vocabs.at(h);
  std::hash<std::string_view> hasher;
  uint64_t hh = hasher(std::string_view(s));
  auto& sh = v.shards[hh % v.nshards];
  size_t si = sh.map.find(hh, std::string_view(s));
  return si == SIZE_MAX ? -1 : sh.map.slots[si].id;
}

int64_t vocab_insert(int64_t h, const std::string& s) {
  Vocab& v = *g_vocabs.at(h);
  std::hash<std::string_view> hasher;
  uint64_t hh = hasher(std::string_view(s));
  auto& sh = v.shards[hh % v.nshards];
  bool found;
  size_t si = sh.map.find_or_insert(hh, std::string_view(s), found);
  if (found) return sh.map.slots[si].id;
  std::string_view sv = sh.arena.add(std::string_view(s));
  sh.map.slots[si].ptr = sv.data();  // repoint off the caller's buffer
  int64_t id = v.base + static_cast<int64_t>(v.by_id.size());
  sh.map.slots[si].id = id;
  v.by_id.push_back(sv);
  v.values.push_back(parse_value_full(sv));
  return id;
}

py::object vocab_get(int64_t h, int64_t id) {
  Vocab& v = *g_vocabs.at(h);
  int64_t k = id - v.base;
  if (k < 0 || k >= static_cast<int64_t>(v.by_id.size()))
    return py::none();
  std::string_view s = v.by_id[k];
  PyObject* u = PyUnicode_DecodeUTF8(s.data(),
                                     static_cast<Py_ssize_t>(s.size()),
                                     "replace");
  return py::reinterpret_steal<py::object>(u);
}

// batch decode for result materialization: CPU int64 id tensor -> Python
// list of str (ids outside the annex range decode to None)
py::list vocab_decode_batch(int64_t h, at::Tensor ids) {
  Vocab& v = *g_vocabs.at(h);
  TORCH_CHECK(!ids.is_cuda() && ids.dtype() == at::kLong);
  const int64_t* r = ids.data_ptr<int64_t>();
  int64_t n = ids.numel();
  py::list out(n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t k = r[i] - v.base;
    PyObject* o;
    if (k < 0 || k >= static_cast<int64_t>(v.by_id.size())) {
      o = Py_None;
      Py_INCREF(o);
    } else {
      std::string_view s = v.by_id[k];
      o = PyUnicode_DecodeUTF8(s.data(),
                               static_cast<Py_ssize_t>(s.size()), "replace");
      if (o == nullptr) { o = Py_None; Py_INCREF(o); }
    }
    PyList_SET_ITEM(out.ptr(), i, o);
  }
  return out;
}

double vocab_value(int64_t h, int64_t id) {
  Vocab& v = *g_vocabs.at(h);
  int64_t k = id - v.base;
  if (k < 0 || k >= static_cast<int64_t>(v.values.size())) return 0.0;
  return v.values[k];
}

at::Tensor vocab_values(int64_t h) {
  Vocab& v = *g_vocabs.at(h);
  return at::from_blob(v.values.data(),
                       {static_cast<int64_t>(v.values.size())},
                       at::kDouble).clone();
}

py::list vocab_export_strings(int64_t h, int64_t start, int64_t count) {
  Vocab& v = *g_vocabs.at(h);
  py::list out;
  int64_t n = static_cast<int64_t>(v.by_id.size());
  for (int64_t k = start; k < std::min(start + count, n); ++k) {
    std::string_view s = v.by_id[k];
    PyObject* u = PyUnicode_DecodeUTF8(
        s.data(), static_cast<Py_ssize_t>(s.size()), "replace");
    out.append(py::reinterpret_steal<py::object>(u));
  }
  return out;
}

// annex terms [start, start+count) packed for the device term-text table:
// (uint8 blob of their concatenated UTF-8, int64 byte length per term),
// copied straight from the by_id views — no Python str objects.  `start`
// is annex-relative (id - base); the range is clamped to the annex.
py::tuple vocab_pack_bytes(int64_t h, int64_t start, int64_t count) {
  Vocab& v = *g_vocabs.at(h);
  int64_t n = static_cast<int64_t>(v.by_id.size());
  int64_t lo = std::min(std::max<int64_t>(start, 0), n);
  int64_t hi = std::min(lo + std::max<int64_t>(count, 0), n);
  auto lens = at::empty({hi - lo}, at::kLong);
  int64_t* lp = lens.data_ptr<int64_t>();
  int64_t total = 0;
  for (int64_t k = lo; k < hi; ++k) {
    lp[k - lo] = static_cast<int64_t>(v.by_id[k].size());
    total += lp[k - lo];
  }
  auto blob = at::empty({total}, at::kByte);
  uint8_t* bp = total ? blob.data_ptr<uint8_t>() : nullptr;
  int64_t at_byte = 0;
  for (int64_t k = lo; k < hi; ++k) {
    std::string_view s = v.by_id[k];
    if (!s.empty()) memcpy(bp + at_byte, s.data(), s.size());
    at_byte += static_cast<int64_t>(s.size());
  }
  return py::make_tuple(blob, lens);
}

// file -> parse -> intern DIRECTLY into the vocab annex (no Python-object
// pass at all); returns (int32 [n,3] global-id rows, fallback lines)
py::tuple parse_ntriples_file_annex(const std::string& path,
                                    int64_t n_threads, int64_t h,
                                    int64_t max_id) {
  const bool dbg = getenv("KOLIBRIE_PARSE_DEBUG") != nullptr;
  auto tick = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!dbg) return;
    auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[annex] %s: %.3fs\n", what,
            std::chrono::duration<double>(now - tick).count());
    tick = now;
  };
  Vocab& voc = *g_vocabs.at(h);
  // the bulky scratch (10 GB file text + per-chunk intern maps with tens
  // of millions of nodes) lives on the heap and is freed by a DETACHED
  // reaper thread after return — its node-by-node teardown takes seconds
  // and would otherwise serialize at scope exit, after all useful work
  struct AnnexScratch {
    const char* map_ptr = nullptr;   // mmap'd input (preferred: no copy)
    size_t map_len = 0;
    std::string text;                // fallback buffer if mmap fails
    std::vector<ParseChunkOut> outs;
    std::vector<std::vector<int64_t>> remaps;
    ~AnnexScratch() {
      if (map_ptr)
        munmap(const_cast<char*>(map_ptr), map_len);
    }
  };
  auto scratch = std::make_unique<AnnexScratch>();
  {
    py::gil_scoped_release release;
    int fd = open(path.c_str(), O_RDONLY);
    TORCH_CHECK(fd >= 0, "cannot open ", path);
    struct stat st {};
    TORCH_CHECK(fstat(fd, &st) == 0, "cannot stat ", path);
    size_t sz = static_cast<size_t>(st.st_size);
    void* m = sz ? mmap(nullptr, sz, PROT_READ, MAP_PRIVATE, fd, 0)
                 : nullptr;
    if (m != nullptr && m != MAP_FAILED) {
      madvise(m, sz, MADV_WILLNEED);
      scratch->map_ptr = static_cast<const char*>(m);
      scratch->map_len = sz;
    } else if (sz) {
      scratch->text.resize(sz);
      size_t off = 0;
      while (off < sz) {
        ssize_t rd = read(fd, scratch->text.data() + off, sz - off);
        TORCH_CHECK(rd > 0, "short read of ", path);
        off += static_cast<size_t>(rd);
      }
    }
    close(fd);
  }
  const char* data = scratch->map_ptr ? scratch->map_ptr
                                      : scratch->text.data();
  lap("read");
  const size_t n = scratch->map_ptr ? scratch->map_len
                                    : scratch->text.size();
  int nt = static_cast<int>(n_threads);
  if (nt <= 0) {
    nt = static_cast<int>(std::thread::hardware_concurrency());
    if (nt <= 0) nt = 8;
  }
  if (nt > 32) nt = 32;
  if (n < (1 << 20)) nt = 1;
  std::vector<size_t> starts(1, 0);
  for (int i = 1; i < nt; ++i) {
    size_t p = n * static_cast<size_t>(i) / nt;
    const char* nl = static_cast<const char*>(
        memchr(data + p, '\n', n - p));
    starts.push_back(nl ? static_cast<size_t>(nl - data) + 1 : n);
  }
  starts.push_back(n);
  scratch->outs.resize(nt);
  scratch->remaps.resize(nt);
  std::vector<ParseChunkOut>& outs = scratch->outs;
  std::vector<std::vector<int64_t>>& remaps = scratch->remaps;
  std::vector<int64_t> line_off(nt + 1, 0);
  int64_t total_rows = 0;
  at::Tensor ids_t;
  {
    py::gil_scoped_release release;
    std::vector<std::thread> threads;
    for (int i = 0; i < nt; ++i)
      threads.emplace_back(parse_chunk_nt, data, starts[i],
                           starts[i + 1], false, std::ref(outs[i]));
    for (auto& t : threads) t.join();
    if (dbg) { py::gil_scoped_acquire a; lap("parallel parse"); }
    for (int i = 0; i < nt; ++i) {
      remaps[i].resize(outs[i].views.size());
      line_off[i + 1] = line_off[i] + outs[i].line_count;
      total_rows += static_cast<int64_t>(outs[i].ids.size());
    }
    // sharded merge straight into the vocab: the vocab's shard count is
    // the parallelism; thread t owns vocab shard t.  Two phases: dedup
    // with PROVISIONAL (shard, local) ids, then per-shard contiguous
    // real-id blocks from prefix sums — no contended atomic, and ids are
    // deterministic for a given input + shard count.
    const int S = voc.nshards;
    std::vector<std::thread> mthreads;
    std::vector<std::vector<std::string_view>> pending(S);
    const int64_t kProv = 1LL << 62;  // provisional marker
    for (int t = 0; t < S; ++t)
      mthreads.emplace_back([&, t]() {
        auto& sh = voc.shards[t];
        auto& pend = pending[t];
        for (int i = 0; i < nt; ++i) {
          auto& views = outs[i].views;
          auto& rm = remaps[i];
          auto& hs = outs[i].hashes;
          for (uint32_t k : outs[i].by_shard[t]) {
            bool found;
            size_t si = sh.map.find_or_insert(hs[k], views[k], found);
            if (found) {
              rm[k] = sh.map.slots[si].id;  // may itself be provisional
              continue;
            }
            std::string_view sv = sh.arena.add(views[k]);
            sh.map.slots[si].ptr = sv.data();  // text/owned die with scratch
            int64_t prov = kProv | (static_cast<int64_t>(t) << 40)
                           | static_cast<int64_t>(pend.size());
            sh.map.slots[si].id = prov;
            pend.push_back(sv);
            rm[k] = prov;
          }
        }
      });
    for (auto& t : mthreads) t.join();
    if (dbg) { py::gil_scoped_acquire a; lap("vocab merge"); }
    // prefix sums -> real id blocks; fix the maps + fill by_id/values
    int64_t old_n = static_cast<int64_t>(voc.by_id.size());
    std::vector<int64_t> shard_base(S + 1, 0);
    for (int t = 0; t < S; ++t)
      shard_base[t + 1] = shard_base[t]
                          + static_cast<int64_t>(pending[t].size());
    int64_t new_total = old_n + shard_base[S];
    TORCH_CHECK(voc.base + new_total <= max_id,
                "dictionary ID space exhausted");
    voc.by_id.resize(new_total);
    voc.values.resize(new_total, 0.0);
    std::vector<std::thread> vthreads;
    for (int t = 0; t < S; ++t)
      vthreads.emplace_back([&, t]() {
        auto& sh = voc.shards[t];
        int64_t base = voc.base + old_n + shard_base[t];
        std::hash<std::string_view> hasher;
        for (size_t j = 0; j < pending[t].size(); ++j) {
          std::string_view sv = pending[t][j];
          int64_t id = base + static_cast<int64_t>(j);
          size_t si = sh.map.find(hasher(sv), sv);
          sh.map.slots[si].id = id;
          int64_t k = id - voc.base;
          voc.by_id[k] = sv;
          voc.values[k] = parse_value_full(sv);
        }
      });
    for (auto& t : vthreads) t.join();
    // resolve provisional remap entries to real ids
    std::vector<std::thread> fthreads;
    for (int i = 0; i < nt; ++i)
      fthreads.emplace_back([&, i]() {
        for (auto& e : remaps[i]) {
          if (e & kProv) {
            int64_t t = (e >> 40) & 0x3FFFFF;
            int64_t j = e & ((1LL << 40) - 1);
            e = voc.base + old_n + shard_base[t] + j;
          }
        }
      });
    for (auto& t : fthreads) t.join();
    // remap rows to global ids, in parallel
    ids_t = at::empty({total_rows / 3, 3}, at::kInt);
    std::vector<int64_t> offs(nt + 1, 0);
    for (int i = 0; i < nt; ++i)
      offs[i + 1] = offs[i] + static_cast<int64_t>(outs[i].ids.size());
    int32_t* dst = ids_t.data_ptr<int32_t>();
    std::vector<std::thread> rthreads;
    for (int i = 0; i < nt; ++i)
      rthreads.emplace_back([&, i]() {
        auto& rm = remaps[i];
        int32_t* d = dst + offs[i];
        for (size_t k = 0; k < outs[i].ids.size(); ++k)
          d[k] = static_cast<int32_t>(
              static_cast<uint32_t>(rm[outs[i].ids[k]]));
      });
    for (auto& t : rthreads) t.join();
    if (dbg) { py::gil_scoped_acquire a; lap("register+remap"); }
  }
  py::list pyfallback;
  for (int i = 0; i < nt; ++i)
    for (auto f : outs[i].fallback) pyfallback.append(f + line_off[i]);
  std::thread([sc = scratch.release()]() { delete sc; }).detach();
  return py::make_tuple(ids_t, pyfallback);
}

py::tuple parse_ntriples_file_mt(const std::string& path,
                                 int64_t n_threads) {
  std::string text;
  {
    py::gil_scoped_release release;
    FILE* f = fopen(path.c_str(), "rb");
    TORCH_CHECK(f != nullptr, "cannot open ", path);
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    text.resize(static_cast<size_t>(sz));
    size_t rd = fread(text.data(), 1, static_cast<size_t>(sz), f);
    fclose(f);
    TORCH_CHECK(rd == static_cast<size_t>(sz), "short read of ", path);
  }
  return parse_nlines_host_mt(text, false, n_threads);
}

// synthetic employee N-Triples FILE generator (bench tooling: writing
// 100M f-string lines from Python costs minutes; this streams the file
// in ~seconds with the same shape as parallel/synthetic.py)
int64_t gen_employee_nt_file(const std::string& path,
                             int64_t total_triples) {
  py::gil_scoped_release release;
  const int64_t n_emp = std::max<int64_t>(1, total_triples / 7);
  const int64_t n_dept = std::max<int64_t>(1, n_emp / 100);
  FILE* f = fopen(path.c_str(), "wb");
  TORCH_CHECK(f != nullptr, "cannot open ", path, " for writing");
  std::vector<char> buf(1 << 22);
  setvbuf(f, buf.data(), _IOFBF, buf.size());
  int64_t lines = 0;
  static const char* kPos[3] = {"Manager", "Developer", "Salesperson"};
  for (int64_t i = 0; i < n_emp; ++i) {
    long e = static_cast<long>(i);
    long d = static_cast<long>(i % n_dept);
    fprintf(f,
            "<http://synthetic/e%ld> <http://xmlns.com/foaf/0.1/name> "
            "\"name%ld\" .\n"
            "<http://synthetic/e%ld> "
            "<http://xmlns.com/foaf/0.1/workplaceHomepage> "
            "<http://synthetic/h%ld> .\n"
            "<http://synthetic/e%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/"
            "annual_salary> \"%ld\" .\n"
            "<http://synthetic/e%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/position> "
            "\"%s\" .\n"
            "<http://synthetic/e%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/email> "
            "\"e%ld@example.org\" .\n"
            "<http://synthetic/e%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/age> "
            "\"%ld\" .\n"
            "<http://synthetic/e%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/worksFor> "
            "<http://synthetic/d%ld> .\n",
            e, e, e, e, e, 30000 + (e * 37) % 120000, e,
            kPos[e % 3], e, e, e, 20 + (e * 13) % 50, e, d);
    lines += 7;
  }
  for (int64_t i = 0; i < n_dept; ++i) {
    long d = static_cast<long>(i);
    fprintf(f,
            "<http://synthetic/d%ld> "
            "<https://data.cityofchicago.org/resource/xzkq-xp2w/locatedIn> "
            "<http://synthetic/c%ld> .\n"
            "<http://synthetic/d%ld> "
            "<http://www.w3.org/2000/01/rdf-schema#label> \"dept %ld\" .\n",
            d, static_cast<long>(i % 1000), d, d);
    lines += 2;
  }
  fclose(f);
  return lines;
}

py::tuple parse_ntriples_host(const std::string& text) {
  return parse_nlines_host(text, false);
}

// N-Quads: optional 4th graph term; absent -> -1 in the id row
// (host bulk replacement for sparql_database.rs:1411 parse_nquads_and_add)
py::tuple parse_nquads_host(const std::string& text) {
  return parse_nlines_host(text, true);
}

// ------------------------------------------------------------ K4: group agg
// Hand-written GROUP BY hash aggregate (replaces reference
// execute_query.rs:404-475 aggregate_rows).
//
// One pass over (key, value) rows into an open-addressing global table,
// staged through a per-workgroup LDS table first: low-cardinality keys
// (the contended case) are pre-aggregated at LDS-atomic speed and flushed
// once per block, so global atomics see at most (#blocks x #groups)
// traffic; high-cardinality keys miss the small LDS table and go straight
// to the (uncontended) global table.  A compaction pass then emits the
// occupied slots.  MIN/MAX on doubles use the monotone bit encoding so
// unsigned 64-bit atomicMin/Max apply.
//
// Keys are caller-packed int64 (single var: (uint32)id; two vars:
// (a<<32)|b).  `empty_key` is a caller-chosen value no row can produce.
constexpr int kAggLdsSlots = 2048;   // 5 x 8 B x 2048 = 80 KiB LDS -> 2 WG/CU

__device__ __forceinline__ uint32_t h64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return static_cast<uint32_t>(k);
}

__device__ __forceinline__ unsigned long long enc_double(double x) {
  unsigned long long b =
      static_cast<unsigned long long>(__double_as_longlong(x));
  return (b & 0x8000000000000000ULL) ? ~b : (b | 0x8000000000000000ULL);
}

__device__ __forceinline__ double dec_double(unsigned long long e) {
  unsigned long long b =
      (e & 0x8000000000000000ULL) ? (e & 0x7FFFFFFFFFFFFFFFULL) : ~e;
  return __longlong_as_double(static_cast<long long>(b));
}

// probe-run cap: at the <=50% load factor the host wrapper guarantees on
// the final attempt, expected linear-probe runs are ~2 slots; a run this
// long means the table is too small — flag overflow and let the host
// re-run bigger.  A full-table scan here (the naive failure mode) would
// cost minutes at millions of threads.
constexpr uint32_t kAggMaxProbe = 128;

__device__ __forceinline__ int64_t agg_claim_slot(
    unsigned long long* __restrict__ keys, uint32_t mask,
    unsigned long long key, unsigned long long empty,
    int32_t* __restrict__ overflow) {
  uint32_t h = h64(key) & mask;
  uint32_t cap = mask < kAggMaxProbe ? mask : kAggMaxProbe;
  for (uint32_t probe = 0; probe <= cap; ++probe) {
    unsigned long long cur = keys[h];
    if (cur == empty) {
      // resolve via CAS, not a re-read: atomics land in L2 and a stale
      // L1 line could keep reporting `empty` forever
      cur = atomicCAS(&keys[h], empty, key);
      if (cur == empty) return h;
    }
    if (cur == key) return h;
    h = (h + 1) & mask;
  }
  atomicExch(overflow, 1);  // table too loaded: caller re-runs bigger
  return -1;
}

__global__ void __launch_bounds__(kBlock)
group_agg_kernel(const int64_t* __restrict__ keys_in,
                 const double* __restrict__ vals, int64_t n,
                 unsigned long long empty,
                 unsigned long long* __restrict__ gkeys,
                 unsigned long long* __restrict__ gcnt,
                 double* __restrict__ gsum,
                 unsigned long long* __restrict__ gmn,
                 unsigned long long* __restrict__ gmx,
                 uint32_t gmask, int32_t* __restrict__ overflow,
                 int use_lds) {
  __shared__ unsigned long long lkeys[kAggLdsSlots];
  __shared__ unsigned long long lcnt[kAggLdsSlots];
  __shared__ double lsum[kAggLdsSlots];
  __shared__ unsigned long long lmn[kAggLdsSlots];
  __shared__ unsigned long long lmx[kAggLdsSlots];
  for (int i = threadIdx.x; i < kAggLdsSlots; i += blockDim.x) {
    lkeys[i] = empty;
    lcnt[i] = 0ULL;
    lsum[i] = 0.0;
    lmn[i] = ~0ULL;
    lmx[i] = 0ULL;
  }
  __syncthreads();
  const bool want_val = vals != nullptr;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if ((i & 0x3FF) == 0 && *overflow) return;  // abort a doomed attempt
    unsigned long long key = static_cast<unsigned long long>(keys_in[i]);
    double v = want_val ? vals[i] : 0.0;
    unsigned long long ev = want_val ? enc_double(v) : 0ULL;
    // LDS attempt: short probe run, then spill to the global table.
    // use_lds=0 (high estimated cardinality: most keys would miss the
    // small LDS table anyway) goes straight to the global table.
    uint32_t h = h64(key) & (kAggLdsSlots - 1);
    int64_t slot = -1;
    for (int p = 0; use_lds && p < 8; ++p) {
      unsigned long long cur = lkeys[h];
      if (cur == key) { slot = h; break; }
      if (cur == empty) {
        unsigned long long prev = atomicCAS(&lkeys[h], empty, key);
        if (prev == empty || prev == key) { slot = h; break; }
        continue;  // re-read: someone else claimed it this cycle
      }
      h = (h + 1) & (kAggLdsSlots - 1);
    }
    if (slot >= 0) {
      atomicAdd(&lcnt[slot], 1ULL);
      if (want_val) {
        if (gsum) atomicAdd(&lsum[slot], v);
        if (gmn) atomicMin(&lmn[slot], ev);
        if (gmx) atomicMax(&lmx[slot], ev);
      }
    } else {
      int64_t gs = agg_claim_slot(gkeys, gmask, key, empty, overflow);
      if (gs < 0) return;
      atomicAdd(&gcnt[gs], 1ULL);
      if (want_val) {
        if (gsum) atomicAdd(&gsum[gs], v);
        if (gmn) atomicMin(&gmn[gs], ev);
        if (gmx) atomicMax(&gmx[gs], ev);
      }
    }
  }
  __syncthreads();
  // flush the block's LDS pre-aggregates into the global table
  for (int i = threadIdx.x; i < kAggLdsSlots; i += blockDim.x) {
    if (lkeys[i] == empty) continue;
    int64_t gs = agg_claim_slot(gkeys, gmask, lkeys[i], empty, overflow);
    if (gs < 0) return;
    atomicAdd(&gcnt[gs], lcnt[i]);
    if (gsum) atomicAdd(&gsum[gs], lsum[i]);
    if (gmn) atomicMin(&gmn[gs], lmn[i]);
    if (gmx) atomicMax(&gmx[gs], lmx[i]);
  }
}

__global__ void agg_compact(const unsigned long long* __restrict__ gkeys,
                            const unsigned long long* __restrict__ gcnt,
                            const double* __restrict__ gsum,
                            const unsigned long long* __restrict__ gmn,
                            const unsigned long long* __restrict__ gmx,
                            int64_t cap, unsigned long long empty,
                            int64_t* __restrict__ out_keys,
                            int64_t* __restrict__ out_cnt,
                            double* __restrict__ out_sum,
                            double* __restrict__ out_mn,
                            double* __restrict__ out_mx,
                            int32_t* __restrict__ counter) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long k = gkeys[i];
    if (k == empty) continue;
    int32_t idx = atomicAdd(counter, 1);
    out_keys[idx] = static_cast<int64_t>(k);
    out_cnt[idx] = static_cast<int64_t>(gcnt[i]);
    if (out_sum) out_sum[idx] = gsum[i];
    if (out_mn) out_mn[idx] = dec_double(gmn[i]);
    if (out_mx) out_mx[idx] = dec_double(gmx[i]);
  }
}

// host wrapper: (keys[n] int64, vals[n] double|None) ->
//   (keys[g], cnt[g], sum[g]|None, min[g]|None, max[g]|None)
py::tuple group_aggregate(at::Tensor keys, c10::optional<at::Tensor> vals,
                          bool want_sum, bool want_min, bool want_max,
                          int64_t empty_key, int64_t groups_hint) {
  TORCH_CHECK(keys.is_cuda() && keys.dtype() == at::kLong && keys.dim() == 1);
  const int64_t n = keys.numel();
  const double* vptr = nullptr;
  if (vals.has_value()) {
    TORCH_CHECK(vals->is_cuda() && vals->dtype() == at::kDouble
                && vals->numel() == n);
    vptr = vals->data_ptr<double>();
  }
  const bool want_val = vptr != nullptr;
  auto opts_i64 = keys.options();
  auto opts_f64 = keys.options().dtype(at::kDouble);
  auto opts_i32 = keys.options().dtype(at::kInt);
  auto stream = cur_stream();
  const unsigned long long empty =
      static_cast<unsigned long long>(empty_key);
  // size from the caller's sampled cardinality estimate (4x the upper
  // bound keeps load <=25%) or default to ~n/4; retry x8 on overflow —
  // the final rung 2*n can never overflow.  A failed attempt aborts
  // early (probe cap + overflow poll), costing ~one extra key pass.
  int64_t cap = 1 << 14;
  if (groups_hint > 0) {
    while (cap < 4 * groups_hint && cap < 2 * n) cap <<= 1;
  } else {
    while (cap < n / 4 && cap < (1LL << 27)) cap <<= 1;
  }
  const bool use_lds =
      groups_hint > 0 ? (groups_hint <= 3000) : true;
  for (;;) {
    auto gkeys = at::full({cap}, empty_key, opts_i64);
    auto gcnt = at::zeros({cap}, opts_i64);
    at::Tensor gsum, gmn, gmx;
    double* gsum_p = nullptr;
    unsigned long long* gmn_p = nullptr;
    unsigned long long* gmx_p = nullptr;
    if (want_val && want_sum) {
      gsum = at::zeros({cap}, opts_f64);
      gsum_p = gsum.data_ptr<double>();
    }
    if (want_val && want_min) {
      gmn = at::full({cap}, -1, opts_i64);  // ~0ULL = +inf in the encoding
      gmn_p = reinterpret_cast<unsigned long long*>(gmn.data_ptr<int64_t>());
    }
    if (want_val && want_max) {
      gmx = at::zeros({cap}, opts_i64);     // 0 = -inf in the encoding
      gmx_p = reinterpret_cast<unsigned long long*>(gmx.data_ptr<int64_t>());
    }
    auto overflow = at::zeros({1}, opts_i32);
    if (n > 0) {
      hipLaunchKernelGGL(group_agg_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                         stream, keys.data_ptr<int64_t>(), vptr, n, empty,
                         reinterpret_cast<unsigned long long*>(
                             gkeys.data_ptr<int64_t>()),
                         reinterpret_cast<unsigned long long*>(
                             gcnt.data_ptr<int64_t>()),
                         gsum_p, gmn_p, gmx_p,
                         static_cast<uint32_t>(cap - 1),
                         overflow.data_ptr<int32_t>(),
                         use_lds ? 1 : 0);
      HIP_OK(hipGetLastError());
    }
    if (n > 0 && overflow.item<int32_t>() != 0) {
      int64_t full = 1;
      while (full < 2 * n) full <<= 1;
      TORCH_CHECK(cap < full, "group_aggregate: overflow at 2*n capacity");
      cap = std::min(cap << 3, full);
      continue;
    }
    auto out_keys = at::empty({cap}, opts_i64);
    auto out_cnt = at::empty({cap}, opts_i64);
    at::Tensor out_sum, out_mn, out_mx;
    double* os = nullptr; double* omn = nullptr; double* omx = nullptr;
    if (gsum_p) { out_sum = at::empty({cap}, opts_f64);
                  os = out_sum.data_ptr<double>(); }
    if (gmn_p) { out_mn = at::empty({cap}, opts_f64);
                 omn = out_mn.data_ptr<double>(); }
    if (gmx_p) { out_mx = at::empty({cap}, opts_f64);
                 omx = out_mx.data_ptr<double>(); }
    auto counter = at::zeros({1}, opts_i32);
    hipLaunchKernelGGL(agg_compact, dim3(grid_for(cap)), dim3(kBlock), 0,
                       stream,
                       reinterpret_cast<unsigned long long*>(
                           gkeys.data_ptr<int64_t>()),
                       reinterpret_cast<unsigned long long*>(
                           gcnt.data_ptr<int64_t>()),
                       gsum_p, gmn_p, gmx_p, cap, empty,
                       out_keys.data_ptr<int64_t>(),
                       out_cnt.data_ptr<int64_t>(), os, omn, omx,
                       counter.data_ptr<int32_t>());
    HIP_OK(hipGetLastError());
    int64_t g = counter.item<int32_t>();
    py::tuple t(5);
    t[0] = out_keys.narrow(0, 0, g);
    t[1] = out_cnt.narrow(0, 0, g);
    t[2] = gsum_p ? py::cast(out_sum.narrow(0, 0, g)) : py::none();
    t[3] = gmn_p ? py::cast(out_mn.narrow(0, 0, g)) : py::none();
    t[4] = gmx_p ? py::cast(out_mx.narrow(0, 0, g)) : py::none();
    return t;
  }
}

// ------------------------------------------------- K6: small-N fixpoint
// Persistent SINGLE-WORKGROUP semi-naive fixpoint for small working sets
// (the deep-taxonomy shape = 10 000 rounds of 1-fact
// deltas, where per-round kernel-launch + host-sync overhead dominates
// any columnar formulation).  One 1024-thread block runs the WHOLE
// fixpoint: rounds are __syncthreads() boundaries (ns, not µs), and all
// inter-thread data passes stay inside one CU so workgroup-scope fences
// suffice (MI355X guide §Workgroup dispatch: no agent-scope traffic).
//
// Rule language (host driver rejects anything else and falls back):
//   kind=1 (join):  (a P1 b), (c P2 d) -> conclusions, exactly ONE shared
//                   var between the premises, predicates constant;
//   kind=0 (copy):  (a P1 b) -> conclusions.
// Conclusions (<=2 per rule): (src_s Pc src_o), srcs in {p1.s,p1.o,p2.s,
// p2.o}.  Covers transitive closure, type propagation (deep taxonomy),
// ancestor programs.
//
// State per predicate (global memory, host-allocated):
//   - pair dedup set: open addressing on packed (s<<32)|o u64, CAS claim;
//   - optional adjacency by-s / by-o: chained hash (heads + append-only
//     {key,val,next} entries), only for directions some rule probes.
// The fact log `out` doubles as the delta queue: [d_lo, d_hi) is the
// current round's delta; appended facts form the next round's.
//
// Ref semantics: datalog semi_naive.rs:17-86 (one-shared-var case).
constexpr int kFxBlock = 1024;
constexpr unsigned long long kFxEmpty = ~0ULL;  // (UNBOUND,UNBOUND) pair

struct FxRule {
  int32_t kind;      // 0 copy, 1 join
  int32_t p1, j1;    // premise1 pred idx; shared-var position (0=s,1=o)
  int32_t p2, j2;    // premise2 (join only)
  int32_t n_conc;
  int32_t c_pred[2];
  int32_t c_s_src[2];  // 0=p1.s 1=p1.o 2=p2.s 3=p2.o
  int32_t c_o_src[2];
};

struct FxPred {
  unsigned long long* set;   // pair dedup table
  uint32_t set_mask;
  int32_t* adj_s_heads; uint32_t adj_s_mask;   // by-subject chains
  int32_t* adj_o_heads; uint32_t adj_o_mask;   // by-object chains
};

struct FxState {
  // shared append-only pools (all predicates)
  int64_t* adj_entries;      // packed (key<<32)|val
  int32_t* adj_next;
  int32_t* adj_pred_dir;     // unused slot kept for debug
  int32_t* out_s; int32_t* out_p; int32_t* out_o;  // fact log (pred idx)
  int32_t* counters;         // [0]=out_n [1]=adj_n [2]=overflow [3]=rounds
  int64_t out_cap, adj_cap;
};

__device__ __forceinline__ bool fx_set_insert(const FxPred& pr,
                                              uint32_t s, uint32_t o,
                                              int32_t* overflow) {
  unsigned long long key =
      (static_cast<unsigned long long>(s) << 32) | o;
  uint32_t h = h64(key) & pr.set_mask;
  uint32_t cap = pr.set_mask < kAggMaxProbe ? pr.set_mask : kAggMaxProbe;
  for (uint32_t p = 0; p <= cap; ++p) {
    unsigned long long cur = pr.set[h];
    if (cur == kFxEmpty) {
      cur = atomicCAS(&pr.set[h], kFxEmpty, key);  // L2 truth, not L1
      if (cur == kFxEmpty) return true;
    }
    if (cur == key) return false;
    h = (h + 1) & pr.set_mask;
  }
  atomicExch(overflow, 1);
  return false;
}

// L1-bypassing relaxed loads: atomic publishes (atomicExch heads,
// atomicAdd counters) land in L2 and never refresh even this CU's own
// L1, so every read of a mutable shared structure goes L2-served.
__device__ __forceinline__ int32_t fx_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int64_t fx_ld64(const int64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Allocation counters / overflow flag / optional LDS delta ring.  In the
// persistent single-WG kernel these live in LDS (per-emit bookkeeping at
// LDS-atomic speed instead of ~4 L2 round trips); the multi-block seed
// kernel passes the global counters instead.
constexpr int kFxRing = 4096;

struct FxCtx {
  int32_t* out_n;
  int32_t* adj_n;
  int32_t* overflow;
  int32_t* ring_s; int32_t* ring_p; int32_t* ring_o;  // LDS or null
  int32_t ring_base;   // fact-log index of ring slot 0 (this round)
};

__device__ __forceinline__ void fx_adj_insert(int32_t* heads, uint32_t mask,
                                              uint32_t key, uint32_t val,
                                              FxCtx& cx, FxState& st) {
  int32_t e = atomicAdd(cx.adj_n, 1);
  if (e >= st.adj_cap) { atomicExch(cx.overflow, 1); return; }
  __hip_atomic_store(
      &st.adj_entries[e],
      static_cast<int64_t>((static_cast<unsigned long long>(key) << 32) | val),
      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // lock-free push: next[e] must hold the correct predecessor BEFORE the
  // head CAS makes e reachable, or a concurrent walker would read junk
  uint32_t h = h32(key) & mask;
  int32_t prev = fx_ld(&heads[h]);
  for (;;) {
    __hip_atomic_store(&st.adj_next[e], prev, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_block();
    int32_t seen = atomicCAS(&heads[h], prev, e);
    if (seen == prev) break;
    prev = seen;
  }
}

// emit one derived fact: dedup -> fact log (= next delta) -> adjacencies
__device__ __forceinline__ void fx_emit(int32_t pidx, uint32_t s, uint32_t o,
                                        const FxPred* preds, FxCtx& cx,
                                        FxState& st) {
  const FxPred& pr = preds[pidx];
  if (!fx_set_insert(pr, s, o, cx.overflow)) return;
  int32_t idx = atomicAdd(cx.out_n, 1);
  if (idx >= st.out_cap) { atomicExch(cx.overflow, 1); return; }
  __hip_atomic_store(&st.out_s[idx], static_cast<int32_t>(s),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st.out_p[idx], pidx,
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st.out_o[idx], static_cast<int32_t>(o),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (cx.ring_s) {
    int32_t r = idx - cx.ring_base;
    if (r >= 0 && r < kFxRing) {
      cx.ring_s[r] = static_cast<int32_t>(s);
      cx.ring_p[r] = pidx;
      cx.ring_o[r] = static_cast<int32_t>(o);
    }
  }
  if (pr.adj_s_heads)
    fx_adj_insert(pr.adj_s_heads, pr.adj_s_mask, s, o, cx, st);
  if (pr.adj_o_heads)
    fx_adj_insert(pr.adj_o_heads, pr.adj_o_mask, o, s, cx, st);
}

__device__ __forceinline__ uint32_t fx_src(int src, uint32_t s1, uint32_t o1,
                                           uint32_t s2, uint32_t o2) {
  switch (src) {
    case 0: return s1;
    case 1: return o1;
    case 2: return s2;
    default: return o2;
  }
}

// compile-time caps so ALL rule/dispatch metadata fits in LDS (a tiny
// few KB): per-round reads of it then cost LDS cycles, not L2 latency —
// at 10 000 one-fact rounds the metadata reads would otherwise dominate
constexpr int kFxMaxRules = 64;
constexpr int kFxMaxPreds = 16;
constexpr int kFxMaxDisp = 128;

__global__ void __launch_bounds__(kFxBlock)
fx_kernel(const FxRule* __restrict__ g_rules, int n_rules,
          const FxPred* __restrict__ g_preds, int n_preds,
          const int32_t* __restrict__ g_disp_off,   // [n_preds+1]
          const int32_t* __restrict__ g_disp_rule,  // rule index
          const int32_t* __restrict__ g_disp_side,  // 0: fact is premise1
          FxState st, int64_t n_init, int64_t adj_seeded,
          int64_t max_rounds) {
  __shared__ int32_t s_dlo, s_dhi, s_use_ring;
  __shared__ int32_t sh_out_n, sh_adj_n, sh_overflow;
  __shared__ FxRule rules[kFxMaxRules];
  __shared__ FxPred preds[kFxMaxPreds];
  __shared__ int32_t disp_off[kFxMaxPreds + 1];
  __shared__ int32_t disp_rule[kFxMaxDisp];
  __shared__ int32_t disp_side[kFxMaxDisp];
  // double-buffered: this round's emits write parity buffer `round & 1`
  // while readers consume the previous round's buffer
  __shared__ int32_t ring_s[2][kFxRing], ring_p[2][kFxRing],
      ring_o[2][kFxRing];
  if (threadIdx.x == 0) {
    s_dlo = 0;
    s_dhi = static_cast<int32_t>(n_init);
    s_use_ring = 0;
    sh_out_n = static_cast<int32_t>(n_init);
    sh_adj_n = static_cast<int32_t>(adj_seeded);
    sh_overflow = 0;
    for (int i = 0; i < n_rules; ++i) rules[i] = g_rules[i];
    for (int i = 0; i < n_preds; ++i) preds[i] = g_preds[i];
    int nd = g_disp_off[n_preds];
    for (int i = 0; i <= n_preds; ++i) disp_off[i] = g_disp_off[i];
    for (int i = 0; i < nd; ++i) {
      disp_rule[i] = g_disp_rule[i];
      disp_side[i] = g_disp_side[i];
    }
  }
  __syncthreads();
  int64_t rounds_done = 0;
  for (int64_t round = 0; round < max_rounds; ++round) {
    int32_t dlo = s_dlo, dhi = s_dhi;
    if (dlo >= dhi) break;
    bool ring_ok = s_use_ring != 0;
    const int wb = static_cast<int>(round & 1), rb = wb ^ 1;
    FxCtx cx{&sh_out_n, &sh_adj_n, &sh_overflow,
             ring_s[wb], ring_p[wb], ring_o[wb], dhi};
    for (int32_t i = dlo + threadIdx.x; i < dhi; i += blockDim.x) {
      uint32_t fs, fo; int32_t fp;
      if (ring_ok) {
        fs = static_cast<uint32_t>(ring_s[rb][i - dlo]);
        fp = ring_p[rb][i - dlo];
        fo = static_cast<uint32_t>(ring_o[rb][i - dlo]);
      } else {
        fs = static_cast<uint32_t>(fx_ld(&st.out_s[i]));
        fp = fx_ld(&st.out_p[i]);
        fo = static_cast<uint32_t>(fx_ld(&st.out_o[i]));
      }
      for (int32_t d = disp_off[fp]; d < disp_off[fp + 1]; ++d) {
        const FxRule& r = rules[disp_rule[d]];
        int side = disp_side[d];
        if (r.kind == 0) {
          for (int c = 0; c < r.n_conc; ++c)
            fx_emit(r.c_pred[c], fx_src(r.c_s_src[c], fs, fo, 0, 0),
                    fx_src(r.c_o_src[c], fs, fo, 0, 0), preds, cx, st);
          continue;
        }
        // join: this fact binds one premise; probe the other's adjacency
        int other_p = side == 0 ? r.p2 : r.p1;
        int my_j = side == 0 ? r.j1 : r.j2;
        int ot_j = side == 0 ? r.j2 : r.j1;
        uint32_t v = my_j == 0 ? fs : fo;   // shared-var value
        const FxPred& op = preds[other_p];
        int32_t* heads = ot_j == 0 ? op.adj_s_heads : op.adj_o_heads;
        uint32_t mask = ot_j == 0 ? op.adj_s_mask : op.adj_o_mask;
        if (!heads) continue;  // driver guarantees presence; safety
        uint32_t h = h32(v) & mask;
        for (int32_t e = fx_ld(&heads[h]); e >= 0;
             e = fx_ld(&st.adj_next[e])) {
          unsigned long long kv =
              static_cast<unsigned long long>(fx_ld64(&st.adj_entries[e]));
          if (static_cast<uint32_t>(kv >> 32) != v) continue;
          uint32_t w = static_cast<uint32_t>(kv);
          uint32_t s2, o2;
          if (ot_j == 0) { s2 = v; o2 = w; } else { s2 = w; o2 = v; }
          uint32_t s1, o1;
          if (side == 0) { s1 = fs; o1 = fo; }
          else { s1 = s2; o1 = o2; s2 = fs; o2 = fo; }
          // (when side==1 the roles swap: this fact IS premise2)
          for (int c = 0; c < r.n_conc; ++c)
            fx_emit(r.c_pred[c], fx_src(r.c_s_src[c], s1, o1, s2, o2),
                    fx_src(r.c_o_src[c], s1, o1, s2, o2), preds, cx, st);
        }
      }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
      s_dlo = dhi;
      int32_t n = sh_out_n;
      if (n > st.out_cap) n = static_cast<int32_t>(st.out_cap);
      s_dhi = n;
      // next round may read its delta from the LDS ring only if EVERY
      // fact appended this round landed in it
      s_use_ring = (n - dhi) <= kFxRing ? 1 : 0;
    }
    __syncthreads();
    rounds_done = round + 1;
    if (sh_overflow) break;  // overflow: host falls back
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    st.counters[0] = sh_out_n;
    st.counters[1] = sh_adj_n;
    st.counters[2] = sh_overflow;
    st.counters[3] = static_cast<int32_t>(rounds_done);
  }
}

// seed kernel: parallel insert of the initial facts (dedup + adjacency)
__global__ void fx_seed(const int32_t* __restrict__ s,
                        const int32_t* __restrict__ p,
                        const int32_t* __restrict__ o, int64_t n,
                        const FxPred* __restrict__ preds, FxState st) {
  FxCtx cx{&st.counters[0], &st.counters[1], &st.counters[2],
           nullptr, nullptr, nullptr, 0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    fx_emit(p[i], static_cast<uint32_t>(s[i]), static_cast<uint32_t>(o[i]),
            preds, cx, st);
  }
}

// host wrapper.  rules_flat: [n_rules,12] int32 rows =
//   kind,p1,j1,p2,j2,n_conc,c0_pred,c0_s,c0_o,c1_pred,c1_s,c1_o
// adj_need: [n_preds,2] bool-ish int32 (by_s, by_o)
// facts: int32 columns with p already mapped to predicate indexes
py::tuple small_fixpoint(at::Tensor rules_flat, at::Tensor adj_need,
                         at::Tensor disp_off, at::Tensor disp_rule,
                         at::Tensor disp_side,
                         at::Tensor fs, at::Tensor fp, at::Tensor fo,
                         int64_t budget, int64_t max_rounds) {
  TORCH_CHECK(fs.is_cuda() && fs.dtype() == at::kInt);
  const int64_t n_init = fs.numel();
  const int n_rules = rules_flat.size(0);
  const int n_preds = adj_need.size(0);
  auto opts_i32 = fs.options();
  auto opts_i64 = fs.options().dtype(at::kLong);
  auto stream = cur_stream();

  // ---- host-side structure assembly (tiny) ----
  auto rules_h = rules_flat.to(at::kCPU).contiguous();
  auto need_h = adj_need.to(at::kCPU).contiguous();
  std::vector<FxRule> rules_v(n_rules);
  const int32_t* rr = rules_h.data_ptr<int32_t>();
  for (int i = 0; i < n_rules; ++i) {
    const int32_t* q = rr + i * 12;
    FxRule& r = rules_v[i];
    r.kind = q[0]; r.p1 = q[1]; r.j1 = q[2]; r.p2 = q[3]; r.j2 = q[4];
    r.n_conc = q[5];
    r.c_pred[0] = q[6]; r.c_s_src[0] = q[7]; r.c_o_src[0] = q[8];
    r.c_pred[1] = q[9]; r.c_s_src[1] = q[10]; r.c_o_src[1] = q[11];
  }
  int64_t set_cap = 64;
  while (set_cap < 2 * (n_init + budget)) set_cap <<= 1;
  int64_t head_cap = 64;
  while (head_cap < n_init + budget) head_cap <<= 1;

  std::vector<at::Tensor> keepalive;
  std::vector<FxPred> preds_v(n_preds);
  const int32_t* nd = need_h.data_ptr<int32_t>();
  for (int i = 0; i < n_preds; ++i) {
    auto set_t = at::full({set_cap}, -1, opts_i64);
    keepalive.push_back(set_t);
    preds_v[i].set = reinterpret_cast<unsigned long long*>(
        set_t.data_ptr<int64_t>());
    preds_v[i].set_mask = static_cast<uint32_t>(set_cap - 1);
    preds_v[i].adj_s_heads = nullptr;
    preds_v[i].adj_o_heads = nullptr;
    preds_v[i].adj_s_mask = preds_v[i].adj_o_mask = 0;
    if (nd[i * 2 + 0]) {
      auto h = at::full({head_cap}, -1, opts_i32);
      keepalive.push_back(h);
      preds_v[i].adj_s_heads = h.data_ptr<int32_t>();
      preds_v[i].adj_s_mask = static_cast<uint32_t>(head_cap - 1);
    }
    if (nd[i * 2 + 1]) {
      auto h = at::full({head_cap}, -1, opts_i32);
      keepalive.push_back(h);
      preds_v[i].adj_o_heads = h.data_ptr<int32_t>();
      preds_v[i].adj_o_mask = static_cast<uint32_t>(head_cap - 1);
    }
  }
  const int64_t out_cap = n_init + budget;
  const int64_t adj_cap = 2 * out_cap;
  auto out_s = at::empty({out_cap}, opts_i32);
  auto out_p = at::empty({out_cap}, opts_i32);
  auto out_o = at::empty({out_cap}, opts_i32);
  auto adj_e = at::empty({adj_cap}, opts_i64);
  auto adj_n = at::empty({adj_cap}, opts_i32);
  auto counters = at::zeros({8}, opts_i32);
  FxState st;
  st.adj_entries = adj_e.data_ptr<int64_t>();
  st.adj_next = adj_n.data_ptr<int32_t>();
  st.adj_pred_dir = nullptr;
  st.out_s = out_s.data_ptr<int32_t>();
  st.out_p = out_p.data_ptr<int32_t>();
  st.out_o = out_o.data_ptr<int32_t>();
  st.counters = counters.data_ptr<int32_t>();
  st.out_cap = out_cap;
  st.adj_cap = adj_cap;

  // device copies of the rule/pred tables
  auto rules_bytes = at::from_blob(rules_v.data(),
      {static_cast<int64_t>(n_rules * sizeof(FxRule))},
      at::TensorOptions().dtype(at::kByte)).clone().to(fs.device());
  auto preds_bytes = at::from_blob(preds_v.data(),
      {static_cast<int64_t>(n_preds * sizeof(FxPred))},
      at::TensorOptions().dtype(at::kByte)).clone().to(fs.device());
  keepalive.push_back(rules_bytes);
  keepalive.push_back(preds_bytes);
  auto d_off = disp_off.to(fs.device(), at::kInt).contiguous();
  auto d_rule = disp_rule.to(fs.device(), at::kInt).contiguous();
  auto d_side = disp_side.to(fs.device(), at::kInt).contiguous();

  const FxPred* dp = reinterpret_cast<const FxPred*>(
      preds_bytes.data_ptr<uint8_t>());
  if (n_init > 0) {
    hipLaunchKernelGGL(fx_seed, dim3(grid_for(n_init)), dim3(kBlock), 0,
                       stream, fs.data_ptr<int32_t>(), fp.data_ptr<int32_t>(),
                       fo.data_ptr<int32_t>(), n_init, dp, st);
    HIP_OK(hipGetLastError());
  }
  // NOTE: the seed pass already appended the init facts to the log; the
  // fixpoint's first delta is [0, counters[0]) == all seeded facts.
  auto seed_cts = counters.to(at::kCPU);
  int64_t seeded = seed_cts[0].item<int32_t>();
  int64_t adj_seeded = seed_cts[1].item<int32_t>();
  TORCH_CHECK(n_rules <= kFxMaxRules && n_preds <= kFxMaxPreds
              && d_rule.numel() <= kFxMaxDisp,
              "small_fixpoint: program exceeds LDS metadata caps");
  hipLaunchKernelGGL(fx_kernel, dim3(1), dim3(kFxBlock), 0, stream,
                     reinterpret_cast<const FxRule*>(
                         rules_bytes.data_ptr<uint8_t>()),
                     n_rules, dp, n_preds, d_off.data_ptr<int32_t>(),
                     d_rule.data_ptr<int32_t>(), d_side.data_ptr<int32_t>(),
                     st, seeded, adj_seeded, max_rounds);
  HIP_OK(hipGetLastError());
  auto cts = counters.to(at::kCPU);
  int32_t n_out = cts[0].item<int32_t>();
  int32_t overflow = cts[2].item<int32_t>();
  int32_t rounds = cts[3].item<int32_t>();
  if (n_out > out_cap) n_out = static_cast<int32_t>(out_cap);
  py::tuple t(6);
  t[0] = out_s.narrow(0, 0, n_out);
  t[1] = out_p.narrow(0, 0, n_out);
  t[2] = out_o.narrow(0, 0, n_out);
  t[3] = py::int_(seeded);
  t[4] = py::int_(overflow);
  t[5] = py::int_(rounds);
  return t;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("small_fixpoint", &small_fixpoint,
        "K6 persistent single-workgroup semi-naive fixpoint for small "
        "working sets (deep-taxonomy class) -> (s, p_idx, o, n_seeded, "
        "overflow, rounds)");
  m.def("group_aggregate", &group_aggregate,
        "K4 LDS-staged hash GROUP BY: (keys, vals?, sum, min, max, empty, "
        "groups_hint) -> (group keys, counts, sums?, mins?, maxs?)");
  m.def("parse_ntriples_host", &parse_ntriples_host,
        "bulk N-Triples parse -> (local-id triples, strings, fallback lines)");
  m.def("parse_nquads_host", &parse_nquads_host,
        "bulk N-Quads parse -> (local-id quads, strings, fallback lines)");
  m.def("parse_ntriples_host_mt", &parse_ntriples_host_mt,
        "multithreaded bulk N-Triples parse (chunk-per-thread + merged "
        "intern tables; GIL released)");
  m.def("parse_nquads_host_mt", &parse_nquads_host_mt,
        "multithreaded bulk N-Quads parse");
  m.def("parse_ntriples_file_mt", &parse_ntriples_file_mt,
        "read + multithreaded-parse an N-Triples file");
  m.def("parse_ntriples_file_encode", &parse_ntriples_file_encode,
        "file -> parallel parse -> intern into the Python dictionary -> "
        "global-id int32 rows");
  m.def("gen_employee_nt_file", &gen_employee_nt_file,
        "write a synthetic employee N-Triples file (bench tooling)");
  m.def("vocab_create", &vocab_create, "native bulk-vocabulary annex");
  m.def("vocab_len", &vocab_len);
  m.def("vocab_lookup", &vocab_lookup);
  m.def("vocab_insert", &vocab_insert);
  m.def("vocab_get", &vocab_get);
  m.def("vocab_decode_batch", &vocab_decode_batch);
  m.def("vocab_value", &vocab_value);
  m.def("vocab_values", &vocab_values);
  m.def("vocab_export_strings", &vocab_export_strings);
  m.def("stats_gather", &stats_gather, "K8 one-pass database statistics");
  m.def("vocab_create_seeded", &vocab_create_seeded,
        "create a vocab annex pre-seeded with the frozen Python prefix");
  m.def("parse_ntriples_file_annex", &parse_ntriples_file_annex,
        "file -> parallel parse -> intern into the native vocab annex");
  m.doc() = "kolibrie_amd native CDNA4 kernels (gfx950)";
  m.def("probe_exact", &probe_exact,
        "K1 scan-probe, packed (a,b) exact keys -> (li, b, z)");
  m.def("probe_range", &probe_range,
        "K1 scan-probe, leading-component range -> (li, b, z)");
  m.def("hash_join", &hash_join,
        "K2 chained hash join over int32 key columns -> (li, ri)");
  m.def("chain_tile", []() { return static_cast<int64_t>(kChainTile); },
        "seed rows per chain tile (win buffer sizing)");
  m.def("probe_sorted_min", []() { return kProbeSortedMin; },
        "fewest probe rows at which a sorted probe column takes the "
        "merge-path count");
  m.def("chain_span", []() { return static_cast<int64_t>(kChainSpan); },
        "widest key span a tile's window is counted by direct address, and "
        "the most window rows a tile stages for the LDS merge");
  m.def("chain_count", &chain_count,
        "fused COUNT(*) over a seed scan + probe-hop chain",
        py::arg("seed_b"), py::arg("seed_z"), py::arg("hop_key32"),
        py::arg("hop_src"), py::arg("hop_table"),
        py::arg("hop_dmin") = std::vector<int64_t>{});
  m.def("chain_count_into", &chain_count_into,
        "allocation/sync-free chain count into caller buffers "
        "(hipGraph-capturable)");
  m.def("register_chain_serve", &register_chain_serve,
        "cache a COUNT chain's launch arguments C++-side; returns handle",
        py::arg("seed_b"), py::arg("seed_z"), py::arg("hop_key32"),
        py::arg("hop_src"), py::arg("hop_table"),
        py::arg("hop_dmin") = std::vector<int64_t>{});
  m.def("serve_chain_count", &serve_chain_count,
        py::call_guard<py::gil_scoped_release>(),
        "one-call serving: direct launches + pinned 8-byte readback");
  m.def("chain_serve_packed", &chain_serve_packed,
        "whether a serve handle took the packed-tile format (6 B per seed)");
  m.def("chain_serve_format", &chain_serve_format,
        "0 = columns, 1 = 6-byte packed tiles, 2 = dense tiles",
        py::arg("id"));
  m.def("chain_serve_decode", &chain_serve_decode,
        "(seed_b, seed_z, row_keys) decoded on the host from a dense "
        "registration's tiles (for tests)", py::arg("id"));
  m.def("release_chain_serve", &release_chain_serve,
        "drop a cached serve handle (store changed)");
  m.def("build_count_table32", &build_count_table32,
        "packed-u32 (val<<7)|count open-addressing table (half the L2 "
        "footprint; requires val < 2^25, count < 128)");
  m.def("build_count_table", &build_count_table,
        "open-addressing (value -> match count) table from packed "
        "(val<<32)|count entries, for hashed chain-count hops");
  m.def("probe_fused", &probe_fused,
        "K1 fused probe: inline key pack + merge-path + carry emit");
  m.def("probe_exact_counts", &probe_exact_counts,
        "K1 count-only exact probe -> per-row match counts");
  m.def("probe_range_counts", &probe_range_counts,
        "K1 count-only range probe -> per-row match counts");
  m.def("hash_join_counts", &hash_join_counts,
        "K2 count-only hash join -> per-left-row match counts");
  m.def("semi_join_mask", &semi_join_mask, py::arg("probe_cols"),
        py::arg("build_cols"), py::arg("anti"), py::arg("lds_tier") = -1,
        "K13 semi join -> uint8 per probe row: has an equal build row, "
        "flipped by anti");
  m.def("left_join", &left_join, py::arg("left_keys"), py::arg("right_keys"),
        py::arg("cond") = py::none(),
        "K14 conditional left outer join -> (li, ri, matched)");
  m.def("left_join_counts", &left_join_counts, py::arg("left_keys"),
        py::arg("right_keys"), py::arg("cond") = py::none(),
        "K14 count-only: pairs per left row that pass the condition");
  m.def("filter_bytecode", &filter_bytecode,
        "K5 filter bytecode evaluation -> bool mask");
  m.def("str_match", &str_match,
        "K9 string predicate over the term-text table -> "
        "(uint8 mask 0/1/2, device overflow-row count)");
  m.def("str_long_threshold",
        []() { return static_cast<int64_t>(kStrLongThreshold); },
        "term length above which CONTAINS rows take the long-term kernel");
  m.def("term_chunk_keys", &term_chunk_keys,
        "K11 7-byte big-endian sort key + count byte of each term at its "
        "depth -> int64 (sign-flipped)");
  m.def("term_adjacent_lcp", &term_adjacent_lcp,
        "K11 common-prefix length of neighbouring terms of one group, "
        "measured from depth -> int64 (sentinel at group heads)");
  m.def("term_lcp_sentinel",
        []() { return static_cast<int64_t>(kLcpSentinel); },
        "value term_adjacent_lcp returns for group heads");
  m.def("term_numeric_class", &term_numeric_class,
        "K11 decimal-literal class per term -> uint8 (0 no, 1 yes, "
        "2 undecided)");
  m.def("path_reach", &path_reach,
        "K12 multi-source BFS over a CSR adjacency, 64 sources per pass -> "
        "(source position, node, per-source counts, self-reach, levels)",
        py::arg("row_ptr"), py::arg("col"), py::arg("sources"),
        py::arg("max_hops"), py::arg("levels_per_sync"),
        py::arg("hub_degree"), py::arg("count_only"));
  m.def("path_reach_batch", []() { return static_cast<int64_t>(kReachBatch); },
        "sources per path_reach pass");
  m.def("vocab_pack_bytes", &vocab_pack_bytes,
        "annex terms packed as (uint8 blob, int64 lengths)");
}
