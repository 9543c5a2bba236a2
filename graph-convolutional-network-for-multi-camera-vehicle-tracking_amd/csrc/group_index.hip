// Stable grouping of int64 keys on the device: index [n_rows] -> perm [n_rows], offsets [n_groups + 1].
// The key of row r is index[r] inside [0, n_groups), else n_groups; perm lists the rows by key, equal keys in increasing
// row order, and group g owns perm[offsets[g] : offsets[g + 1]].  It is what torch.sort(stable=True) + searchsorted gave
// pool.group_by_index, as three to four launches that read nothing back, allocate nothing and can be captured; the
// consumers are mtmc_pool_tracklets_weighted (perm, offsets) and mtmc_scatter_grouped (scatter_ops.hip).
//
// An LSD radix sort over ceil(bits(n_groups) / digit_bits) passes of digit_bits <= 11 bits.  The rows are cut into tiles of
// kGroupTile rows, one workgroup of four waves per tile; wave w owns rows [256 w, 256 w + 256) of its tile, 64 at a time.
// Per pass:
//   group_hist_kernel    table[digit][tile] = rows of the tile with that digit (integer atomics in LDS: counts have no order)
//   group_scan_*         exclusive scan of the table read as one array, digit-major: where the rows of (digit, tile) start.
//                        Up to kScanOneLevel entries one workgroup walks it with a carry; above, every 2048-entry block
//                        scans itself and leaves its total, the same one-workgroup walk scans the totals, and the placement
//                        adds the two (a table of 25 M entries, 100 M rows at 8 bits, is 12 207 totals)
//   group_place_kernel   every row's rank among the equal digits of its tile is COMPUTED: for a wave's 64 rows, in row order,
//                        __ballot over the digit's bits leaves the 64-bit mask of the lanes that share the lane's digit;
//                        rank = the set bits below the lane, count = all of them.  The waves then take turns in wave
//                        order on the tile's running offsets in LDS (read the offset, the first lane of each digit adds the
//                        count), so rows of one digit keep their row order across waves, and across tiles by the scan.
//                        No rank is drawn from the return value of an atomic.
// One pass (n_groups + 1 <= 2^digit_bits: the pool's case) reads index and writes perm, and the offsets are the scanned
// digit totals, written by tile 0.  With more passes (key, row) pairs of 32 bits each ping-pong in the workspace (keys and
// rows are < 2^31), the last pass writes perm and the sorted keys, and offsets[g] is the first position whose key is >= g
// (a binary search per group: one launch, nothing to clear).  Only masked digits of a key ever index anything.
#include "api_error.h"
#include "kernels.h"
#include <limits.h>

namespace mtmc {

constexpr int kGroupTile = 1024;          // rows per tile (mtmc_group_tile_rows)
constexpr int kGroupMaxBits = 11;         // widest digit: 2048 bins, 8 KiB of LDS
constexpr int kScanBlock = 2048;          // entries per workgroup and trip of the scans: 8 per thread
constexpr int64_t kScanOneLevel = 4096;   // tables up to this many entries: one workgroup, no totals

template <bool FIRST>
__device__ __forceinline__ unsigned group_key(const int64_t* index, const unsigned* keys, int64_t r, int64_t n_groups) {
  if (FIRST) {
    const int64_t v = index[r];
    return (unsigned)((v >= 0 && v < n_groups) ? v : n_groups);
  }
  return keys[r];
}

template <bool FIRST>
__global__ __launch_bounds__(256) void group_hist_kernel(const int64_t* index, const unsigned* keys, int64_t n_rows,
                                                         int64_t n_groups, int shift, int bits, int64_t tiles, unsigned* table) {
  __shared__ unsigned bins[1 << kGroupMaxBits];
  const int nb = 1 << bits;
  for (int d = threadIdx.x; d < nb; d += 256) bins[d] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kGroupTile;
  for (int i = threadIdx.x; i < kGroupTile; i += 256) {
    const int64_t r = r0 + i;
    if (r < n_rows) atomicAdd(&bins[(group_key<FIRST>(index, keys, r, n_groups) >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < nb; d += 256) table[(int64_t)d * tiles + blockIdx.x] = bins[d];   // (zeros too: no memset)
}

// Exclusive scan of data[i0 .. i0 + 2048) (entries past n count 0) by one workgroup of 256 threads, in place, starting at
// `carry`; returns the sum of the 2048 entries in every thread.  wtot: 4 words of LDS.
__device__ __forceinline__ unsigned group_scan_2048(unsigned* data, int64_t i0, int64_t n, unsigned carry, unsigned* wtot) {
  const int64_t at = i0 + (int64_t)threadIdx.x * 8;
  unsigned v[8], mine = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = at + k < n ? data[at + k] : 0u;
    mine += v[k];
  }
  unsigned incl = mine;                                    // inclusive scan of `mine` over the wave's 64 lanes
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned up = __shfl_up(incl, m, 64);
    if (lane >= m) incl += up;
  }
  if (lane == 63) wtot[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned before = carry, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned t = wtot[w];
    if (w < (int)(threadIdx.x >> 6)) before += t;
    total += t;
  }
  unsigned run = before + incl - mine;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (at + k < n) data[at + k] = run;
    run += v[k];
  }
  __syncthreads();                                         // (wtot is free for the next trip)
  return total;
}

__global__ __launch_bounds__(256) void group_scan_blocks_kernel(unsigned* data, int64_t n, unsigned* sums) {
  __shared__ unsigned wtot[4];
  const unsigned total = group_scan_2048(data, (int64_t)blockIdx.x * kScanBlock, n, 0u, wtot);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the whole array, 2048 entries a trip, the running total carried from trip to trip
__global__ __launch_bounds__(256) void group_scan_serial_kernel(unsigned* data, int64_t n) {
  __shared__ unsigned wtot[4];
  unsigned carry = 0;
  for (int64_t i0 = 0; i0 < n; i0 += kScanBlock) carry += group_scan_2048(data, i0, n, carry, wtot);
}

// FIRST: keys from index, rows are the row numbers; else the (key, row) pairs of the pass before.  LAST: rows go to perm.
// offsets != NULL (the only pass): tile 0 writes offsets[0 .. n_groups] and info from the scanned digit totals.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void group_place_kernel(const int64_t* index, const unsigned* keys_in, const unsigned* rows_in,
                                                          int64_t n_rows, int64_t n_groups, int shift, int bits, int64_t tiles,
                                                          const unsigned* table, const unsigned* sums, unsigned* keys_out,
                                                          unsigned* rows_out, int64_t* perm, int64_t* offsets, int* info) {
  __shared__ unsigned base[1 << kGroupMaxBits];
  const int nb = 1 << bits;
  for (int d = threadIdx.x; d < nb; d += 256) {
    const int64_t i = (int64_t)d * tiles + blockIdx.x;
    base[d] = table[i] + (sums ? sums[i / kScanBlock] : 0u);
  }
  __syncthreads();
  if (offsets && blockIdx.x == 0) {                        // (n_groups + 1 <= nb: one pass)
    for (int64_t d = threadIdx.x; d <= n_groups; d += 256) offsets[d] = base[d];
    if (info && threadIdx.x == 0) *info = (int)(n_rows - (int64_t)base[n_groups]);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * kGroupTile + wave * 256;
  unsigned key[4], row[4], digit[4], rank[4], count[4], pos[4];
  bool valid[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t r = w0 + s * 64 + lane;
    valid[s] = r < n_rows;
    key[s] = valid[s] ? group_key<FIRST>(index, keys_in, r, n_groups) : 0u;
    row[s] = FIRST ? (unsigned)r : (valid[s] ? rows_in[r] : 0u);
    digit[s] = (key[s] >> shift) & (nb - 1);
    unsigned long long same = __ballot(valid[s]);          // the lanes whose digit is this lane's
    for (int b = 0; b < bits; ++b) {
      const bool one = (digit[s] >> b) & 1;
      const unsigned long long ones = __ballot(one);
      same &= one ? ones : ~ones;
    }
    rank[s] = __popcll(same & ((1ull << lane) - 1ull));
    count[s] = __popcll(same);
    pos[s] = 0;
  }
  __syncthreads();                                         // (tile 0 has read the digit totals)
  volatile unsigned* run = base;                           // where the next row of each digit goes
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const unsigned at = valid[s] ? run[digit[s]] : 0u;
        pos[s] = at + rank[s];
        if (valid[s] && rank[s] == 0) run[digit[s]] = at + count[s];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!valid[s] || (int64_t)pos[s] >= n_rows) continue;  // (the second: never, by the counts)
    if (LAST) perm[pos[s]] = (int64_t)row[s]; else rows_out[pos[s]] = row[s];
    if (keys_out) keys_out[pos[s]] = key[s];
  }
}

// more than one pass: offsets[g] = the first position of the sorted keys with a key >= g, g = 0 .. n_groups
__global__ __launch_bounds__(256) void group_offsets_kernel(const unsigned* sorted, int64_t n_rows, int64_t n_groups,
                                                            int64_t* offsets, int* info) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g <= n_groups; g += stride) {
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)sorted[mid] < g) lo = mid + 1; else hi = mid;
    }
    offsets[g] = lo;
    if (info && g == n_groups) *info = (int)(n_rows - lo);
  }
}

// without rows or without groups: perm in row order, offsets all 0, every row keyed n_groups
__global__ __launch_bounds__(256) void group_trivial_kernel(int64_t n_rows, int64_t n_groups, int64_t* perm, int64_t* offsets,
                                                            int* info) {
  const int64_t stride = (int64_t)gridDim.x * 256, n = n_rows > n_groups + 1 ? n_rows : n_groups + 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (i < n_rows) perm[i] = i;
    if (i <= n_groups) offsets[i] = 0;
  }
  if (info && blockIdx.x == 0 && threadIdx.x == 0) *info = (int)n_rows;
}

// host side: the digit width and the passes, the workspace
struct GroupPlan {
  int bits, passes;
  int64_t tiles, entries, totals;          // of the table; totals = 0: the one-level scan
  size_t table, sums, pairs[4], bytes;     // offsets into the workspace: keys A, rows A, keys B, rows B
};

static bool group_plan(int64_t n_rows, int64_t n_groups, int32_t digit_bits, GroupPlan* p) {
  if (n_rows < 0 || n_rows >= (1ll << 31) || n_groups < 0 || n_groups >= (1ll << 31) || digit_bits < 0 ||
      digit_bits > kGroupMaxBits)
    return false;
  int need = 1;                                            // bits that hold the keys 0 .. n_groups
  while ((1ll << need) < n_groups + 1) ++need;
  p->tiles = (n_rows + kGroupTile - 1) / kGroupTile;
  int b = digit_bits;
  if (b == 0) {      // the widest digit whose table stays small beside the rows: 11 bits up to 4096 tiles (4 M rows), else 8
    const int cap = p->tiles <= 4096 ? kGroupMaxBits : 8;
    const int passes = (need + cap - 1) / cap;
    b = (need + passes - 1) / passes;
  }
  p->bits = b;
  p->passes = (need + b - 1) / b;
  p->entries = p->tiles << b;
  p->totals = p->entries > kScanOneLevel ? (p->entries + kScanBlock - 1) / kScanBlock : 0;
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t off = 0;
  p->table = off; off += al((size_t)p->entries * sizeof(unsigned));
  p->sums = off; off += al((size_t)p->totals * sizeof(unsigned));
  for (int i = 0; i < 4; ++i) {
    p->pairs[i] = off;
    if (p->passes > 1) off += al((size_t)n_rows * sizeof(unsigned));
  }
  p->bytes = off + 256;                                    // (never 0 for a size the entry takes)
  return true;
}

}  // namespace mtmc

extern "C" {

int32_t mtmc_group_tile_rows(void) { return mtmc::kGroupTile; }

size_t mtmc_group_by_index_workspace_bytes(int64_t n_rows, int64_t n_groups, int32_t digit_bits) {
  mtmc::GroupPlan p;
  return mtmc::group_plan(n_rows, n_groups, digit_bits, &p) ? p.bytes : 0;
}

int32_t mtmc_group_by_index(const int64_t* index, int64_t n_rows, int64_t n_groups, int32_t digit_bits, int64_t* perm,
                            int64_t* offsets, int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace mtmc;
  using mtmc_api::fail;
  GroupPlan p;
  if (!group_plan(n_rows, n_groups, digit_bits, &p))
    return fail(MTMC_E_ARG, "group_by_index: n_rows and n_groups must be in [0, 2^31), digit_bits in [0, %d]", kGroupMaxBits);
  if (!offsets || (n_rows > 0 && (!index || !perm))) return fail(MTMC_E_ARG, "group_by_index: NULL index, perm or offsets");
  if ((((uintptr_t)index | (uintptr_t)perm | (uintptr_t)offsets) & 7) || ((uintptr_t)info & 3))
    return fail(MTMC_E_ARG, "group_by_index: index, perm and offsets must be 8-byte, info 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* inf = reinterpret_cast<int*>(info);
  if (n_rows == 0 || n_groups == 0) {
    const int64_t n = n_rows > n_groups + 1 ? n_rows : n_groups + 1;
    hipLaunchKernelGGL(group_trivial_kernel, dim3(blocks_for(n, 256, 4096)), dim3(256), 0, s, n_rows, n_groups, perm, offsets, inf);
    return mtmc_api::launched("group_by_index");
  }
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < p.bytes)
    return fail(MTMC_E_ARG, "group_by_index: workspace (16-byte aligned) has %zu bytes, %zu needed (mtmc_group_by_index_workspace_bytes)",
                workspace_bytes, p.bytes);
  char* ws = static_cast<char*>(workspace);
  unsigned* table = reinterpret_cast<unsigned*>(ws + p.table);
  unsigned* sums = p.totals ? reinterpret_cast<unsigned*>(ws + p.sums) : nullptr;
  unsigned* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = reinterpret_cast<unsigned*>(ws + p.pairs[i]);
  const dim3 grid((unsigned)p.tiles), wg(256);
  for (int pass = 0; pass < p.passes; ++pass) {
    const bool first = pass == 0, last = pass == p.passes - 1;
    const int shift = pass * p.bits;
    const unsigned *kin = first ? nullptr : buf[2 * ((pass - 1) & 1)], *rin = first ? nullptr : buf[2 * ((pass - 1) & 1) + 1];
    unsigned *kout = p.passes > 1 ? buf[2 * (pass & 1)] : nullptr, *rout = last ? nullptr : buf[2 * (pass & 1) + 1];
    if (first) hipLaunchKernelGGL(group_hist_kernel<true>, grid, wg, 0, s, index, kin, n_rows, n_groups, shift, p.bits, p.tiles, table);
    else hipLaunchKernelGGL(group_hist_kernel<false>, grid, wg, 0, s, index, kin, n_rows, n_groups, shift, p.bits, p.tiles, table);
    if (p.totals) {
      hipLaunchKernelGGL(group_scan_blocks_kernel, dim3((unsigned)p.totals), wg, 0, s, table, p.entries, sums);
      hipLaunchKernelGGL(group_scan_serial_kernel, dim3(1), wg, 0, s, sums, p.totals);
    } else {
      hipLaunchKernelGGL(group_scan_serial_kernel, dim3(1), wg, 0, s, table, p.entries);
    }
    int64_t* off1 = p.passes == 1 ? offsets : nullptr;
#define MTMC_GROUP_PLACE(F, L)                                                                                          \
  hipLaunchKernelGGL((group_place_kernel<F, L>), grid, wg, 0, s, index, kin, rin, n_rows, n_groups, shift, p.bits, p.tiles, \
                     (const unsigned*)table, (const unsigned*)sums, kout, rout, perm, off1, inf)
    if (first && last) MTMC_GROUP_PLACE(true, true);
    else if (first) MTMC_GROUP_PLACE(true, false);
    else if (last) MTMC_GROUP_PLACE(false, true);
    else MTMC_GROUP_PLACE(false, false);
#undef MTMC_GROUP_PLACE
  }
  if (p.passes > 1)
    hipLaunchKernelGGL(group_offsets_kernel, dim3(blocks_for(n_groups + 1, 256, 4096)), wg, 0, s,
                       (const unsigned*)buf[2 * ((p.passes - 1) & 1)], n_rows, n_groups, offsets, inf);
  return mtmc_api::launched("group_by_index");
}

}  // extern "C"
