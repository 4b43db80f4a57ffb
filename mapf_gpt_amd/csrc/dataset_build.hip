// dataset_build.hip -- the device side of the dataset builder: exact duplicate filtering of 256-byte
// token rows through a hash table that carries over between calls, the "wait in goal" balancing of
// dataset/generate_dataset.py:80-95, stable compaction of a keep mask into an index list and a row gather by index list.
//
// Everything the caller can observe is a function of the input alone: the atomics of the insert pass race for slots, but a
// hash owns exactly one slot whoever wins, and the slot's representative is the minimum of the row indices that carry the hash.
// No kernel here uses floating point, scratch, LDS beyond a few KB (the resolve pass: 32 KB) or inline assembly.
#include "common.h"

using namespace mgpt;

namespace {

constexpr int ROW = MGPT_CONTEXT;             // bytes per row
constexpr int TILE = 4096;                    // flags per workgroup in the counting / scanning passes: 256 threads x 16 bytes
constexpr int MAX_COLL_ROWS = 1 << 16;        // collision rows one call may hand to the resolve pass
constexpr int MAX_COLL_SURV = 4096;           // first occurrences that are not their hash's representative, over the set's life
constexpr int64_t MAX_CAPACITY = (int64_t)1 << 28;

__device__ __forceinline__ uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ bool eq16(const uint4 &a, const uint4 &b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// 16 flag bytes from p[i0 .. i0 + 16) as four words, zero beyond n; one 16-byte load where the pointer allows it
__device__ __forceinline__ uint4 load_flags16(const uint8_t *p, int64_t i0, int64_t n, bool aligned)
{
    uint4 w = make_uint4(0, 0, 0, 0);
    if (i0 >= n) return w;
    if (aligned && i0 + 16 <= n) return *reinterpret_cast<const uint4 *>(p + i0);
    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (i0 + j < n) v[j >> 2] |= (uint32_t)p[i0 + j] << (8 * (j & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ uint32_t word_of(const uint4 &w, int k) { return k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w; }
__device__ __forceinline__ uint32_t byte_of(const uint4 &w, int j) { return (word_of(w, j >> 2) >> (8 * (j & 3))) & 0xFFu; }

// exclusive prefix of v over the 256 threads of the workgroup, in thread order; *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *total)
{
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                    // s_wave may still be read by a previous call
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    *total = all;
    return before + inc - v;
}

// ---------------------------------------------------------------------------------------------------------------------
// (a) one 64-bit hash per row: 16 lanes x 16 bytes, four rows = 1 KiB contiguous per wave instruction
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_row_hash_kernel(const uint8_t *__restrict__ rows, int64_t n, uint64_t mask, uint64_t *__restrict__ hashes)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    uint64_t v = 0;
    if (row < n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(rows + row * ROW + l * 16);
        const uint64_t a = (uint64_t)q.x | ((uint64_t)q.y << 32), b = (uint64_t)q.z | ((uint64_t)q.w << 32);
        const uint64_t c = 0x9E3779B97F4A7C15ull * (uint64_t)(2 * l + 1);      // depends on the lane's place in the row
        uint64_t x = (a ^ c) * 0xD6E8FEB86659FD93ull;
        x ^= x >> 32;
        x = (x + (b ^ (c >> 1) ^ 0xA0761D6478BD642Full)) * 0xE7037ED1A0B428DBull;
        x ^= x >> 29;
        v = x;
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 16);
    if (row < n && l == 0) {
        uint64_t h = fmix64(v) & mask;
        if (h == 0) h = 0x9E3779B97F4A7C15ull;                                 // 0 marks an empty slot
        hashes[row] = h;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) insert: one lane per row, linear probing.  A hash claims the first slot of its probe sequence that is empty or already
// its own (slots are never released, so every lane carrying the hash ends at the same slot); the slot's value is the minimum
// global index (rows of the store count from 0, row i of the batch is base + i) of the rows that carry it.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_insert_kernel(const uint64_t *__restrict__ hashes, int64_t n, uint32_t base, unsigned long long *keys,
                                                        uint32_t *vals, uint32_t slot_mask, int shift, uint32_t *__restrict__ slot_of, int *err)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long h = hashes[i];
    const uint32_t g = base + (uint32_t)i;
    uint32_t s = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> shift) & slot_mask;
    for (uint32_t p = 0; p <= slot_mask; p++, s = (s + 1) & slot_mask) {
        unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) cur = atomicCAS(&keys[s], 0ull, h);
        if (cur == 0 || cur == h) {
            if (__hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > g) atomicMin(&vals[s], g);
            slot_of[i] = s;
            return;
        }
    }
    slot_of[i] = 0;             // unreachable while slots >= 2 x capacity; reported, never silently wrong
    atomicOr(err, 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// (c) classify: 16 lanes compare the row with its hash's representative
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_classify_kernel(const uint8_t *__restrict__ rows, int64_t n, uint32_t base, const uint8_t *__restrict__ store,
                                                          const uint32_t *__restrict__ vals, const uint32_t *__restrict__ slot_of,
                                                          uint8_t *__restrict__ first, uint8_t *__restrict__ coll)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15, lane = threadIdx.x & 63;
    bool eq = true, is_rep = false;
    if (row < n) {
        const uint32_t rep = vals[slot_of[row]], g = base + (uint32_t)row;
        is_rep = rep == g;
        if (!is_rep) {
            const uint8_t *p = rep < base ? store + (int64_t)rep * ROW : rows + (int64_t)(rep - base) * ROW;
            const uint4 x = *reinterpret_cast<const uint4 *>(rows + row * ROW + l * 16);
            const uint4 y = *reinterpret_cast<const uint4 *>(p + l * 16);
            eq = eq16(x, y);
        }
    }
    const unsigned long long b = __ballot(eq);
    const bool all_eq = ((b >> (lane & 48)) & 0xFFFFull) == 0xFFFFull;
    if (row < n && l == 0) {
        first[row] = is_rep ? 1 : 0;
        coll[row] = (!is_rep && !all_eq) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// (d) resolve: collision rows (same hash as their representative, other bytes) in index order, one workgroup.  Each is compared
// with the earlier first occurrences of its hash that are not the representative: the persistent list surv_* (global index
// and hash), which this pass extends.  err: 2 = too many collision rows, 4 = list full.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_resolve_kernel(const uint8_t *__restrict__ rows, uint32_t base, const uint8_t *__restrict__ store,
                                                         const uint64_t *__restrict__ hashes, const int64_t *__restrict__ cidx,
                                                         const int64_t *__restrict__ ccount, uint8_t *first, uint32_t *surv_idx,
                                                         uint64_t *surv_hash, int *surv_count, int *err)
{
    __shared__ uint64_t s_hash[MAX_COLL_SURV];
    const int tid = threadIdx.x;
    const int64_t nc = *ccount;
    int ns = *surv_count;
    if (nc == 0) return;
    if (nc > MAX_COLL_ROWS) {
        if (tid == 0) atomicOr(err, 2);
        return;
    }
    for (int j = tid; j < ns; j += 256) s_hash[j] = surv_hash[j];
    __syncthreads();
    for (int64_t c = 0; c < nc; c++) {
        const int64_t i = cidx[c];
        const uint64_t h = hashes[i];
        const uint8_t *mine = rows + i * ROW;
        int found = 0;
        for (int j = tid; j < ns; j += 256) {
            if (s_hash[j] != h) continue;
            const uint32_t e = surv_idx[j];
            const uint8_t *p = e < base ? store + (int64_t)e * ROW : rows + (int64_t)(e - base) * ROW;
            bool same = true;
            for (int k = 0; k < 16 && same; k++)
                same = eq16(*reinterpret_cast<const uint4 *>(mine + k * 16), *reinterpret_cast<const uint4 *>(p + k * 16));
            if (same) found = 1;
        }
        if (!__syncthreads_or(found)) {                 // uniform: a new first occurrence
            if (ns >= MAX_COLL_SURV) {
                if (tid == 0) atomicOr(err, 4);
                return;
            }
            if (tid == 0) {
                surv_idx[ns] = base + (uint32_t)i;
                surv_hash[ns] = h;
                s_hash[ns] = h;
                first[i] = 1;
            }
            ns++;
        }
        __syncthreads();                                // the new entry (LDS and global) is visible to the next row's scan
    }
    if (tid == 0) *surv_count = ns;
}

// first occurrences -> the store (row r of the index list lands at base + r), and the table / list entries that still name the
// batch row are pointed at its place in the store
__global__ __launch_bounds__(256) void ds_append_kernel(const uint8_t *__restrict__ rows, const int64_t *__restrict__ idx, int64_t n_first, uint32_t base,
                                                        uint8_t *__restrict__ store, uint32_t *vals, const uint32_t *__restrict__ slot_of)
{
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n_first) return;
    const int64_t i = idx[r];
    *reinterpret_cast<uint4 *>(store + ((int64_t)base + r) * ROW + l * 16) = *reinterpret_cast<const uint4 *>(rows + i * ROW + l * 16);
    if (l == 0) {
        const uint32_t s = slot_of[i];
        if (vals[s] == base + (uint32_t)i) vals[s] = base + (uint32_t)r;      // one writer per slot: the representative; r <= i
    }
}

__global__ __launch_bounds__(256) void ds_fixup_kernel(uint32_t *surv_idx, const int *surv_count, const int64_t *__restrict__ idx, int64_t n_first, uint32_t base)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= *surv_count || surv_idx[e] < base) return;
    const int64_t i = surv_idx[e] - base;
    int64_t lo = 0, hi = n_first - 1;                   // idx increases; i is in it
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < i) lo = mid + 1; else hi = mid;
    }
    surv_idx[e] = base + (uint32_t)lo;
}

__global__ void ds_counts_kernel(int64_t *counts, int64_t n, int64_t n_first, int64_t n_coll, int64_t total)
{
    if (threadIdx.x == 0) { counts[0] = n_first; counts[1] = n - n_first; counts[2] = n_coll; counts[3] = total; }
}

// ---------------------------------------------------------------------------------------------------------------------
// stable compaction of a byte mask: per-tile counts, one workgroup scans them, tiles scatter in order.  No atomics.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_select_count_kernel(const uint8_t *__restrict__ keep, int64_t n, int aligned, int *__restrict__ tile_count)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint4 w = load_flags16(keep, i0, n, aligned != 0);
    int c = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) c += byte_of(w, j) != 0;
    int total;
    block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// exclusive scan of n_tiles counts (int32 -> int64), in tile order; *total_out = the sum
__global__ __launch_bounds__(256) void ds_tile_scan_kernel(const int *__restrict__ tile_count, int64_t n_tiles, int64_t *__restrict__ tile_off, int64_t *total_out)
{
    __shared__ int64_t s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int64_t t0 = 0; t0 < n_tiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int v = t < n_tiles ? tile_count[t] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        if (t < n_tiles) tile_off[t] = s_run + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = s_run;
}

__global__ __launch_bounds__(256) void ds_select_scatter_kernel(const uint8_t *__restrict__ keep, int64_t n, int aligned, const int64_t *__restrict__ tile_off,
                                                                int64_t *__restrict__ index)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint4 w = load_flags16(keep, i0, n, aligned != 0);
    int c = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) c += byte_of(w, j) != 0;
    int total;
    int64_t o = tile_off[blockIdx.x] + block_exclusive_scan(c, &total);
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (byte_of(w, j) != 0) index[o++] = i0 + j;
}

// ---------------------------------------------------------------------------------------------------------------------
// balance (generate_dataset.py:80-95 in closed form).  Tile counts: [t][0..5] first occurrences per label, [t][6] = those of
// other labels (refused by the host wrapper's caller: labels are 0..5).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ds_balance_count_kernel(const uint8_t *__restrict__ first, const int8_t *__restrict__ labels, int64_t n, int aligned,
                                                               int *__restrict__ tile_count)
{
    __shared__ unsigned long long s_lo[4], s_hi[4];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint4 f = load_flags16(first, i0, n, aligned & 1);
    const uint4 y = load_flags16(reinterpret_cast<const uint8_t *>(labels), i0, n, (aligned & 2) != 0);
    // four 16-bit fields per word: labels 0..3 in lo, 4, 5 and "other" in hi; a tile holds 4096 rows, so no field overflows
    unsigned long long lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (byte_of(f, j) == 0) continue;
        const uint32_t lab = byte_of(y, j);
        if (lab < 4) lo += 1ull << (16 * lab);
        else hi += 1ull << (16 * (lab < 6 ? lab - 4 : 2));
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        lo += __shfl_xor(lo, m);
        hi += __shfl_xor(hi, m);
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x < 8) {
        const unsigned long long a = s_lo[0] + s_lo[1] + s_lo[2] + s_lo[3], b = s_hi[0] + s_hi[1] + s_hi[2] + s_hi[3];
        const int k = threadIdx.x;
        tile_count[(int64_t)blockIdx.x * 8 + k] = k == 7 ? 0 : (int)(((k < 4 ? a : b) >> (16 * (k & 3))) & 0xFFFFull);
    }
}

// one workgroup: totals per label, the exclusive scan of the label-5 tile counts, k, the counters.
// stats int64[10] = {discarded, duplicates, kept, actions_made[0..5] as the reference prints them, labels outside 0..5}
__global__ __launch_bounds__(256) void ds_balance_plan_kernel(const int *__restrict__ tile_count, int64_t n_tiles, int64_t n, int64_t *__restrict__ tile_off5,
                                                              int64_t *__restrict__ stats, int64_t *keep5)
{
    __shared__ int64_t s_run5;
    __shared__ long long s_tot[7];
    if (threadIdx.x < 7) s_tot[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_run5 = 0;
    __syncthreads();
    for (int64_t t0 = 0; t0 < n_tiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int v = t < n_tiles ? tile_count[t * 8 + 5] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        if (t < n_tiles) tile_off5[t] = s_run5 + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_run5 += total;
        if (threadIdx.x < 7) {                          // seven lanes sum one column each: fixed order
            long long a = 0;
            const int64_t t1 = t0 + 256 < n_tiles ? t0 + 256 : n_tiles;
            for (int64_t u = t0; u < t1; u++) a += tile_count[u * 8 + threadIdx.x];
            s_tot[threadIdx.x] += a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int64_t ns = 0;
        for (int k = 0; k < 7; k++) ns += s_tot[k];
        const int64_t n5 = s_tot[5], z = s_tot[0] + n5;
        // smallest k with k == n5 or (z - k) <= (ns - k) / 5; (z - k) - (ns - k) / 5 does not increase with k
        int64_t lo = 0, hi = n5;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (z - mid <= (ns - mid) / 5) hi = mid; else lo = mid + 1;
        }
        const int64_t k = lo;
        stats[0] = k; stats[1] = n - ns; stats[2] = ns - k;
        for (int a = 0; a < 5; a++) stats[3 + a] = s_tot[a];
        stats[8] = n5 - k;
        stats[9] = s_tot[6];
        *keep5 = n5 - k;                                // the first (n5 - k) label-5 survivors stay (as label 0)
    }
}

__global__ __launch_bounds__(256) void ds_balance_apply_kernel(const uint8_t *__restrict__ first, const int8_t *__restrict__ labels, int64_t n, int aligned,
                                                               const int64_t *__restrict__ tile_off5, const int64_t *__restrict__ keep5,
                                                               uint8_t *__restrict__ keep, int8_t *__restrict__ labels_out)
{
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint4 f = load_flags16(first, i0, n, aligned & 1);
    const uint4 y = load_flags16(reinterpret_cast<const uint8_t *>(labels), i0, n, (aligned & 2) != 0);
    int c = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) c += byte_of(f, j) != 0 && byte_of(y, j) == 5;
    int total;
    int64_t rank5 = tile_off5[blockIdx.x] + block_exclusive_scan(c, &total);
    const int64_t stay = *keep5;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (i0 + j >= n) break;
        const bool fo = byte_of(f, j) != 0;
        const uint32_t lab = byte_of(y, j);
        bool k = fo;
        if (fo && lab == 5) k = rank5++ < stay;
        keep[i0 + j] = k ? 1 : 0;
        labels_out[i0 + j] = (int8_t)(lab == 5 ? 0 : lab);
    }
}

// rows and labels by index list: 16 lanes x 16 B per row.  An index outside [0, n_src) gives a zero row with label -1.
__global__ __launch_bounds__(256) void ds_gather_kernel(const uint8_t *__restrict__ rows, const int8_t *__restrict__ labels, int64_t n_src,
                                                        const int64_t *__restrict__ idx, int64_t n_out, uint8_t *__restrict__ rows_out,
                                                        int8_t *__restrict__ labels_out)
{
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (r >= n_out) return;
    const int64_t i = idx[r];
    const bool ok = i >= 0 && i < n_src;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *reinterpret_cast<const uint4 *>(rows + i * ROW + l * 16);
    *reinterpret_cast<uint4 *>(rows_out + r * ROW + l * 16) = v;
    if (l == 0 && labels_out) labels_out[r] = ok ? labels[i] : (int8_t)-1;
}

inline int64_t n_tiles_of(int64_t n) { return cdiv64(n > 0 ? n : 1, TILE); }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned rows16_blocks(int64_t n) { return (unsigned)cdiv64(n * 16, 256); }

// workspace of the scanning passes: [n_tiles][8] int32 tile counts | [n_tiles] int64 tile offsets | one int64
inline int64_t work_bytes(int64_t n) { return n_tiles_of(n) * (8 * 4 + 8) + 64; }

int select_launch(const uint8_t *d_keep, int64_t n, int64_t *d_index, int64_t *d_count, void *d_work, hipStream_t s)
{
    const int64_t nt = n_tiles_of(n);
    int *tile_count = (int *)d_work;
    int64_t *tile_off = (int64_t *)((char *)d_work + nt * 32);
    const int al = aligned16(d_keep) ? 1 : 0;
    ProfScope ps(P_DS_SELECT, s);
    hipLaunchKernelGGL(ds_select_count_kernel, dim3((unsigned)nt), dim3(256), 0, s, d_keep, n, al, tile_count);
    hipLaunchKernelGGL(ds_tile_scan_kernel, dim3(1), dim3(256), 0, s, tile_count, nt, tile_off, d_count);
    hipLaunchKernelGGL(ds_select_scatter_kernel, dim3((unsigned)nt), dim3(256), 0, s, d_keep, n, al, tile_off, d_index);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

}  // namespace

struct mgpt_dedup {
    int64_t capacity = 0, slots = 0, count = 0;       // count: rows in the store (host copy; every filter call ends synchronised)
    int hash_bits = 64, shift = 0, n_surv = 0;
    uint64_t mask = ~0ull;
    bool poisoned = false;                            // a call failed after it had touched the table: reset first
    unsigned long long *keys = nullptr;               // [slots] hash, 0 = empty
    uint32_t *vals = nullptr;                         // [slots] representative (store position once the call is over)
    uint8_t *store = nullptr;                         // [capacity][256] first occurrences so far
    uint64_t *hashes = nullptr;                       // per call: [capacity]
    uint32_t *slot_of = nullptr;
    uint8_t *coll = nullptr;
    int64_t *cidx = nullptr, *idx = nullptr;
    uint32_t *surv_idx = nullptr;                     // [MAX_COLL_SURV]
    uint64_t *surv_hash = nullptr;
    int64_t *scal = nullptr;                          // device: [0] first count, [1] collision rows, [2] int surv_count, [3] int err
    void *work = nullptr;
    DeviceArena mem;                                  // every device pointer above
};

extern "C" int mgpt_dedup_reset(mgpt_dedup *d, void *stream)
{
    MGPT_REQUIRE(d, MGPT_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    MGPT_HIP(hipMemsetAsync(d->keys, 0, (size_t)d->slots * 8, s));
    MGPT_HIP(hipMemsetAsync(d->vals, 0xFF, (size_t)d->slots * 4, s));
    MGPT_HIP(hipMemsetAsync(d->scal, 0, 4 * 8, s));
    d->count = 0;
    d->n_surv = 0;
    d->poisoned = false;
    return MGPT_OK;
}

extern "C" int mgpt_dedup_create(mgpt_dedup **out, int64_t capacity_rows, int hash_bits, void *stream)
{
    MGPT_REQUIRE(out, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(capacity_rows > 0 && capacity_rows <= MAX_CAPACITY, MGPT_ERR_ARG, "capacity_rows=%lld outside 1 .. %lld",
                 (long long)capacity_rows, (long long)MAX_CAPACITY);
    MGPT_REQUIRE(hash_bits >= 1 && hash_bits <= 64, MGPT_ERR_ARG, "hash_bits=%d outside 1 .. 64", hash_bits);
    mgpt_dedup *d = new mgpt_dedup();
    d->capacity = capacity_rows;
    d->hash_bits = hash_bits;
    d->mask = hash_bits == 64 ? ~0ull : ((1ull << hash_bits) - 1);
    int lg = 1;
    while (((int64_t)1 << lg) < 2 * capacity_rows) lg++;
    d->slots = (int64_t)1 << lg;
    d->shift = 64 - lg;
    const size_t cap = (size_t)capacity_rows;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto **p, size_t bytes) { if (e == hipSuccess) e = d->mem.alloc(p, bytes); };
    alloc(&d->keys, (size_t)d->slots * 8);
    alloc(&d->vals, (size_t)d->slots * 4);
    alloc(&d->store, cap * ROW);
    alloc(&d->hashes, cap * 8);
    alloc(&d->slot_of, cap * 4);
    alloc(&d->coll, cap);
    alloc(&d->cidx, cap * 8);
    alloc(&d->idx, cap * 8);
    alloc(&d->surv_idx, MAX_COLL_SURV * 4);
    alloc(&d->surv_hash, MAX_COLL_SURV * 8);
    alloc(&d->scal, 4 * 8);
    alloc(&d->work, (size_t)work_bytes(capacity_rows));
    if (e != hipSuccess) {
        set_error("device allocation failed for a set of %lld rows: %s", (long long)capacity_rows, hipGetErrorString(e));
        delete d;
        return MGPT_ERR_HIP;
    }
    const int rc = mgpt_dedup_reset(d, stream);
    if (rc != MGPT_OK) { delete d; return rc; }
    *out = d;
    return MGPT_OK;
}

extern "C" int mgpt_dedup_destroy(mgpt_dedup *d)
{
    delete d;                                         // (its arena frees what it holds)
    return MGPT_OK;
}

extern "C" int mgpt_dedup_count(const mgpt_dedup *d, int64_t *rows)
{
    MGPT_REQUIRE(d && rows, MGPT_ERR_ARG, "NULL argument");
    *rows = d->count;
    return MGPT_OK;
}

extern "C" int mgpt_dedup_filter(mgpt_dedup *d, const uint8_t *d_rows, int64_t n, uint8_t *d_first, int64_t *d_counts, void *stream)
{
    MGPT_REQUIRE(d && d_rows && d_first, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(n >= 0, MGPT_ERR_ARG, "n=%lld", (long long)n);
    MGPT_REQUIRE(aligned16(d_rows), MGPT_ERR_ARG, "d_rows must be 16-byte aligned");
    MGPT_REQUIRE(d->count + n <= d->capacity, MGPT_ERR_ARG, "%lld rows in the set + %lld new ones exceed its capacity of %lld",
                 (long long)d->count, (long long)n, (long long)d->capacity);
    MGPT_REQUIRE(!d->poisoned, MGPT_ERR_STATE, "an earlier call failed half-way: mgpt_dedup_reset first");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t base = (uint32_t)d->count;
    int64_t h_scal[4] = {0, 0, 0, 0};
    if (n > 0) {
        int *surv_count = (int *)(d->scal + 2), *err = (int *)(d->scal + 3);
        {
            ProfScope ps(P_DS_HASH, s);
            hipLaunchKernelGGL(ds_row_hash_kernel, dim3(rows16_blocks(n)), dim3(256), 0, s, d_rows, n, d->mask, d->hashes);
        }
        {
            ProfScope ps(P_DS_INSERT, s);
            hipLaunchKernelGGL(ds_insert_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, d->hashes, n, base, d->keys, d->vals,
                               (uint32_t)(d->slots - 1), d->shift, d->slot_of, err);
        }
        {
            ProfScope ps(P_DS_CLASSIFY, s);
            hipLaunchKernelGGL(ds_classify_kernel, dim3(rows16_blocks(n)), dim3(256), 0, s, d_rows, n, base, d->store, d->vals, d->slot_of,
                               d_first, d->coll);
        }
        MGPT_LAUNCH_CHECK();
        d->poisoned = true;                           // until the call has gone through
        int rc = select_launch(d->coll, n, d->cidx, d->scal + 1, d->work, s);
        if (rc != MGPT_OK) return rc;
        {
            ProfScope ps(P_DS_RESOLVE, s);
            hipLaunchKernelGGL(ds_resolve_kernel, dim3(1), dim3(256), 0, s, d_rows, base, d->store, d->hashes, d->cidx, d->scal + 1, d_first,
                               d->surv_idx, d->surv_hash, surv_count, err);
        }
        MGPT_LAUNCH_CHECK();
        rc = select_launch(d_first, n, d->idx, d->scal + 0, d->work, s);
        if (rc != MGPT_OK) return rc;
        MGPT_HIP(hipMemcpyAsync(h_scal, d->scal, sizeof(h_scal), hipMemcpyDeviceToHost, s));
        MGPT_HIP(hipStreamSynchronize(s));
        const int h_err = (int)(h_scal[3] & 0xFFFFFFFF), h_surv = (int)(h_scal[2] & 0xFFFFFFFF);
        MGPT_REQUIRE(!(h_err & 1), MGPT_ERR_STATE, "the hash table has no free slot (internal error)");
        MGPT_REQUIRE(!(h_err & 2), MGPT_ERR_UNSUPPORTED, "%lld rows share their hash with a different row: more than the exact pass takes (%d); "
                     "the set must be reset", (long long)h_scal[1], MAX_COLL_ROWS);
        MGPT_REQUIRE(!(h_err & 4), MGPT_ERR_UNSUPPORTED, "more than %d distinct rows collide with another row's hash; the set must be reset",
                     MAX_COLL_SURV);
        const int64_t n_first = h_scal[0];
        if (n_first > 0) {
            ProfScope ps(P_DS_GATHER, s);
            hipLaunchKernelGGL(ds_append_kernel, dim3(rows16_blocks(n_first)), dim3(256), 0, s, d_rows, d->idx, n_first, base, d->store, d->vals,
                               d->slot_of);
        }
        if (h_surv > d->n_surv)
            hipLaunchKernelGGL(ds_fixup_kernel, dim3(cdiv(h_surv, 256)), dim3(256), 0, s, d->surv_idx, surv_count, d->idx, n_first, base);
        MGPT_LAUNCH_CHECK();
        d->n_surv = h_surv;
        d->count += n_first;
        d->poisoned = false;
    }
    if (d_counts) {
        hipLaunchKernelGGL(ds_counts_kernel, dim3(1), dim3(64), 0, s, d_counts, n, h_scal[0], h_scal[1], d->count);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

extern "C" int mgpt_rows_workspace_bytes(int64_t n, int64_t *bytes)
{
    MGPT_REQUIRE(bytes && n >= 0, MGPT_ERR_ARG, "bad argument");
    *bytes = work_bytes(n);
    return MGPT_OK;
}

extern "C" int mgpt_dataset_balance(const uint8_t *d_first, const int8_t *d_labels, int64_t n, uint8_t *d_keep, int8_t *d_labels_out,
                                    int64_t *d_stats, void *d_work, void *stream)
{
    MGPT_REQUIRE(d_first && d_labels && d_keep && d_labels_out && d_stats && d_work, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(n >= 0 && n <= MAX_CAPACITY, MGPT_ERR_ARG, "n=%lld", (long long)n);
    MGPT_REQUIRE(aligned16(d_work), MGPT_ERR_ARG, "d_work must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nt = n_tiles_of(n);
    int *tile_count = (int *)d_work;
    int64_t *tile_off5 = (int64_t *)((char *)d_work + nt * 32), *keep5 = tile_off5 + nt;
    const int al = (aligned16(d_first) ? 1 : 0) | (aligned16(d_labels) ? 2 : 0);
    ProfScope ps(P_DS_BALANCE, s);
    hipLaunchKernelGGL(ds_balance_count_kernel, dim3((unsigned)nt), dim3(256), 0, s, d_first, d_labels, n, al, tile_count);
    hipLaunchKernelGGL(ds_balance_plan_kernel, dim3(1), dim3(256), 0, s, tile_count, nt, n, tile_off5, d_stats, keep5);
    hipLaunchKernelGGL(ds_balance_apply_kernel, dim3((unsigned)nt), dim3(256), 0, s, d_first, d_labels, n, al, tile_off5, keep5, d_keep,
                       d_labels_out);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

extern "C" int mgpt_rows_select(const uint8_t *d_keep, int64_t n, int64_t *d_index, int64_t *d_count, void *d_work, void *stream)
{
    MGPT_REQUIRE(d_keep && d_index && d_count && d_work, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(n >= 0 && n <= MAX_CAPACITY, MGPT_ERR_ARG, "n=%lld", (long long)n);
    MGPT_REQUIRE(aligned16(d_work), MGPT_ERR_ARG, "d_work must be 16-byte aligned");
    return select_launch(d_keep, n, d_index, d_count, d_work, (hipStream_t)stream);
}

extern "C" int mgpt_rows_gather(const uint8_t *d_rows, const int8_t *d_labels, int64_t n_src, const int64_t *d_index, int64_t n_out,
                                uint8_t *d_rows_out, int8_t *d_labels_out, void *stream)
{
    MGPT_REQUIRE(n_out >= 0 && n_src >= 0, MGPT_ERR_ARG, "n_src=%lld n_out=%lld", (long long)n_src, (long long)n_out);
    if (n_out == 0) return MGPT_OK;
    MGPT_REQUIRE(d_rows && d_index && d_rows_out && (!d_labels_out || d_labels), MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(aligned16(d_rows) && aligned16(d_rows_out), MGPT_ERR_ARG, "row buffers must be 16-byte aligned");
    MGPT_REQUIRE(n_out <= MAX_CAPACITY, MGPT_ERR_ARG, "n_out=%lld", (long long)n_out);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(P_DS_GATHER, s);
    hipLaunchKernelGGL(ds_gather_kernel, dim3(rows16_blocks(n_out)), dim3(256), 0, s, d_rows, d_labels, n_src, d_index, n_out, d_rows_out,
                       d_labels_out);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}
