// bmx_kernels13.h -- bit-vectors built from lists of bit positions on the device: bvector::set(ids, n, sort_order) on an empty
// vector, i.e. import / import_sorted / import_block (src/bm.h:4153, 4312, 4364, 4430).  gfx950, wave64.
//
// Nothing here stages a dense bitmap of the vector: memory and time follow the ids and the blocks they touch.
//   1. k_ids_scan     one pass over the ids: largest id, "ids decrease somewhere", block changes per 4,096-id chunk
//      k_ids_reduce   ... over the chunks
//   sorted ids (checked, never trusted):
//   2. k_tbl_part / k_tbl_top / k_tbl_apply   exclusive scan of the chunk counts
//   3. k_ids_starts   the touched blocks in block order: (block, first id) per run of one block's ids
//   any other order: a bucket sort by block that keeps the 16-bit in-block offsets only
//   2'. k_ids_hist[_lds]     ids per block of the shard (in LDS for shards of <= 16,384 blocks)
//   3'. k_tbl_*              scan of the histogram: bucket starts and the touched blocks in block order
//   4'. k_ids_scatter[_lds]  the offsets into their buckets
//   then, over the touched blocks only (the rest of the descriptor table is a memset to NULL):
//   5. k_ids_stats    one wave per touched block: its ids ORed into an 8 KiB image in LDS, popcount / runs / first bit and the
//                     storage decision of k_block_stats (bit-block without optimize; FULL / GAP (< 1,276 runs) / bit with it)
//   6. k_scan_layout  (bmx_kernels.h) over the compacted stats
//   7. k_ids_emit     the image rebuilt, written as a bit-block or converted to GAP exactly as k_emit_blocks writes it
// The table of a vector does not depend on the order of the ids: both paths visit the touched blocks in block order.
#pragma once
#include "bmx_kernels.h"

#define IDS_CHUNK 4096u          // ids per workgroup of k_ids_scan / k_ids_starts (256 threads x 16)
#define TBL_PER   4096u          // entries per workgroup of the k_tbl_* scan (256 threads x 16)

template <class T> __device__ __forceinline__ u32 id_off(T v) { return (u32)v & 0xFFFFu; }

// step 1.  Per 4,096-id chunk c: cmax[c] = its largest id; starts[c] = its ids whose block differs from their predecessor's (the
// first id counts: the runs of a sorted list) | 1 << 31 where an id is smaller than its predecessor.  No global atomics: one
// address hit by every wave of a 1e8-id list serialised the first form (1.1 ms for 1e8 ids, 0.36 TB/s)
template <class T>
__global__ __launch_bounds__(256)
void k_ids_scan(const T* __restrict__ ids, u64 n, u32* __restrict__ starts, u64* __restrict__ cmax)
{
    __shared__ u64 smx[4];
    __shared__ u32 scnt[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u64 base = (u64)blockIdx.x * IDS_CHUNK;
    u64 mx = 0; u32 down = 0, cnt = 0;
#pragma unroll 4
    for (u32 k = 0; k < IDS_CHUNK / 256u; ++k) {
        const u64 i = base + k * 256u + tid;
        if (i < n) {
            const u64 v = (u64)ids[i];
            const u64 p = i ? (u64)ids[i - 1] : v;
            mx = v > mx ? v : mx;
            down |= v < p;
            cnt += (i == 0) || ((v >> 16) != (p >> 16));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { u64 x = __shfl_xor(mx, o, 64); mx = x > mx ? x : mx; }
    cnt = wave_sum(cnt);
    const bool any_down = __ballot(down != 0u) != 0ull;
    if (lane == 0) { smx[w] = mx; scnt[w] = cnt | (any_down ? 0x80000000u : 0u); }
    __syncthreads();
    if (tid == 0) {
        u64 m = smx[0]; u32 c = 0, f = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) { m = smx[j] > m ? smx[j] : m; c += scnt[j] & 0x7FFFFFFFu; f |= scnt[j] & 0x80000000u; }
        cmax[blockIdx.x] = m; starts[blockIdx.x] = c | f;
    }
}

// step 1b, one workgroup: info[0] = the largest id, info[1] = 1 where the list decreases somewhere; the flags leave starts[]
__global__ __launch_bounds__(1024)
void k_ids_reduce(u32* __restrict__ starts, const u64* __restrict__ cmax, u32 nchunks, u64* __restrict__ info)
{
    __shared__ u64 smx[16];
    __shared__ u32 sfl[16];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    u64 mx = 0; u32 f = 0;
    for (u32 c = tid; c < nchunks; c += 1024u) {
        const u64 m = cmax[c]; const u32 s = starts[c];
        mx = m > mx ? m : mx; f |= s >> 31;
        starts[c] = s & 0x7FFFFFFFu;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { u64 x = __shfl_xor(mx, o, 64); mx = x > mx ? x : mx; }
    const bool any = __ballot(f != 0u) != 0ull;
    if (lane == 0) { smx[w] = mx; sfl[w] = any; }
    __syncthreads();
    if (tid == 0) {
        u64 m = 0; u32 a = 0;
        for (u32 j = 0; j < 16; ++j) { m = smx[j] > m ? smx[j] : m; a |= sfl[j]; }
        info[0] = m; info[1] = a;
    }
}

// exclusive scan of u32 entries in three launches (<= 256 x 4,096 = 2^20 entries: chunks of 2^32 ids, blocks of a vector).
// part[wg] = {sum, non-zero entries} of workgroup wg's 4,096 entries; thread t owns entries [t*16, t*16 + 16) of them
__device__ __forceinline__ void tbl_wg_scan(u32 s, u32 z, u32* sm, u32& ps, u32& pz, u32& ts, u32& tz)
{
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u32 is = wave_scan_incl(s, lane), iz = wave_scan_incl(z, lane);
    if (lane == 63u) { sm[w] = is; sm[4 + w] = iz; }
    __syncthreads();
    u32 os = 0, oz = 0; ts = 0; tz = 0;
#pragma unroll
    for (u32 j = 0; j < 4; ++j) { if (j < w) { os += sm[j]; oz += sm[4 + j]; } ts += sm[j]; tz += sm[4 + j]; }
    ps = os + is - s; pz = oz + iz - z;
}

__global__ __launch_bounds__(256)
void k_tbl_part(const u32* __restrict__ in, u32 n, uint2* __restrict__ part)
{
    __shared__ u32 sm[8];
    const u32 b0 = blockIdx.x * TBL_PER + threadIdx.x * 16u;
    u32 s = 0, z = 0;
#pragma unroll
    for (u32 j = 0; j < 16u; ++j) { const u32 i = b0 + j; const u32 v = i < n ? in[i] : 0u; s += v; z += v != 0u; }
    u32 ps, pz, ts, tz;
    tbl_wg_scan(s, z, sm, ps, pz, ts, tz);
    if (threadIdx.x == 0) part[blockIdx.x] = make_uint2(ts, tz);
}

// one workgroup: part[] -> exclusive offsets; totals = {sum, non-zero entries}; with a touched-block list, its sentinel
// tbeg[non-zero entries] = sum (the end of the last bucket)
__global__ __launch_bounds__(256)
void k_tbl_top(uint2* __restrict__ part, u32 nparts, u32* __restrict__ totals, u32* __restrict__ tbeg)
{
    __shared__ u32 sm[8];
    const u32 t = threadIdx.x;
    const uint2 p = t < nparts ? part[t] : make_uint2(0u, 0u);
    u32 ps, pz, ts, tz;
    tbl_wg_scan(p.x, p.y, sm, ps, pz, ts, tz);
    if (t < nparts) part[t] = make_uint2(ps, pz);
    if (t == 0) { totals[0] = ts; totals[1] = tz; if (tbeg) tbeg[tz] = ts; }
}

// out[i] = exclusive prefix of in[] (may alias in); with tblk: every non-zero entry i appends (i + blk0, its prefix) to the
// touched-block list, in entry order
__global__ __launch_bounds__(256)
void k_tbl_apply(const u32* in, u32 n, const uint2* __restrict__ part, u32* out, u32 blk0,
                 u32* __restrict__ tblk, u32* __restrict__ tbeg)
{
    __shared__ u32 sm[8];
    const u32 b0 = blockIdx.x * TBL_PER + threadIdx.x * 16u;
    u32 v[16], s = 0, z = 0;
#pragma unroll
    for (u32 j = 0; j < 16u; ++j) { const u32 i = b0 + j; v[j] = i < n ? in[i] : 0u; s += v[j]; z += v[j] != 0u; }
    u32 ps, pz, ts, tz;
    tbl_wg_scan(s, z, sm, ps, pz, ts, tz);
    const uint2 p = part[blockIdx.x];
    ps += p.x; pz += p.y;
#pragma unroll
    for (u32 j = 0; j < 16u; ++j) {
        const u32 i = b0 + j;
        if (i >= n) break;
        if (out) out[i] = ps;
        if (tblk && v[j]) { tblk[pz] = i + blk0; tbeg[pz] = ps; ++pz; }
        ps += v[j];
    }
}

// step 3 (sorted ids): every id whose block differs from its predecessor's starts a run: tblk[r] = its block, tbeg[r] = its
// index, r = the run's rank (chunk offset from the scan + rank inside the chunk, taken in id order); tbeg[runs] = n
template <class T>
__global__ __launch_bounds__(256)
void k_ids_starts(const T* __restrict__ ids, u64 n, const u32* __restrict__ chunk_off, const u32* __restrict__ totals,
                  u32* __restrict__ tblk, u32* __restrict__ tbeg)
{
    __shared__ u32 sm[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u64 base = (u64)blockIdx.x * IDS_CHUNK;
    u32 r = chunk_off[blockIdx.x];
    for (u32 k = 0; k < IDS_CHUNK / 256u; ++k) {
        const u64 i = base + k * 256u + tid;
        if (base + k * 256u >= n) break;                    // (workgroup-uniform)
        bool st = false; u64 v = 0;
        if (i < n) {
            v = (u64)ids[i];
            st = i == 0 || ((v >> 16) != ((u64)ids[i - 1] >> 16));
        }
        const u64 m = __ballot(st);
        if (lane == 0) sm[w] = (u32)__popcll(m);
        __syncthreads();
        u32 before = 0, all = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) { if (j < w) before += sm[j]; all += sm[j]; }
        if (st) {
            const u32 pos = r + before + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
            tblk[pos] = (u32)(v >> 16); tbeg[pos] = (u32)i;
        }
        r += all;
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) tbeg[totals[0]] = (u32)n;
}

// step 2' (any order): ids per block of the shard [blk0, blk0 + nbl)
template <class T>
__global__ __launch_bounds__(256)
void k_ids_hist(const T* __restrict__ ids, u64 n, u32 blk0, u32 nbl, u32* __restrict__ cnt)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 b = (u64)ids[i] >> 16;
        if (b >= blk0 && b - blk0 < nbl) atomicAdd(&cnt[b - blk0], 1u);
    }
}

// step 4': each in-shard id's offset into its block's bucket; cnt[] counts down to zero on the way
template <class T>
__global__ __launch_bounds__(256)
void k_ids_scatter(const T* __restrict__ ids, u64 n, u32 blk0, u32 nbl, const u32* __restrict__ bstart, u32* __restrict__ cnt,
                   u16* __restrict__ bucket)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 v = (u64)ids[i], b = v >> 16;
        if (b >= blk0 && b - blk0 < nbl) {
            const u32 pos = atomicSub(&cnt[b - blk0], 1u) - 1u;
            bucket[bstart[b - blk0] + pos] = (u16)(v & 0xFFFFu);
        }
    }
}

// steps 2' and 4' for shards of <= IDS_LDS_BLOCKS blocks: the histogram lives in LDS (dynamic, 4 B per block).  Workgroup g owns
// ids [g * per, (g + 1) * per).  Histogram: LDS atomics, then one global atomic per (workgroup, block).  Scatter: the workgroup
// counts its ids again, reserves its stretch of every bucket with one global atomic on cursor[] (zero before), and scatters
// with LDS atomics.  (1e8 shuffled ids over 15,259 blocks: one global atomic per id took 2.6 ms per kernel.)
#define IDS_LDS_BLOCKS 16384u
template <class T>
__device__ __forceinline__ void ids_lds_count(const T* __restrict__ ids, u64 lo, u64 hi, u32 blk0, u32 nbl, u32* h)
{
    for (u32 j = threadIdx.x; j < nbl; j += blockDim.x) h[j] = 0u;
    __syncthreads();
    for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const u64 b = (u64)ids[i] >> 16;
        if (b >= blk0 && b - blk0 < nbl) atomicAdd(&h[b - blk0], 1u);
    }
    __syncthreads();
}

template <class T>
__global__ __launch_bounds__(256)
void k_ids_hist_lds(const T* __restrict__ ids, u64 n, u64 per, u32 blk0, u32 nbl, u32* __restrict__ cnt)
{
    extern __shared__ u32 h[];
    const u64 lo = (u64)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    ids_lds_count(ids, lo, hi, blk0, nbl, h);
    for (u32 j = threadIdx.x; j < nbl; j += blockDim.x)
        if (h[j]) atomicAdd(&cnt[j], h[j]);
}

template <class T>
__global__ __launch_bounds__(256)
void k_ids_scatter_lds(const T* __restrict__ ids, u64 n, u64 per, u32 blk0, u32 nbl, const u32* __restrict__ bstart,
                       u32* __restrict__ cursor, u16* __restrict__ bucket)
{
    extern __shared__ u32 h[];
    const u64 lo = (u64)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    ids_lds_count(ids, lo, hi, blk0, nbl, h);
    for (u32 j = threadIdx.x; j < nbl; j += blockDim.x)
        if (h[j]) h[j] = bstart[j] + atomicAdd(&cursor[j], h[j]);
    __syncthreads();
    for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const u64 v = (u64)ids[i], b = v >> 16;
        if (b >= blk0 && b - blk0 < nbl) bucket[atomicAdd(&h[b - blk0], 1u)] = (u16)(v & 0xFFFFu);
    }
}

// the GAP writer of k_emit_blocks (bmx_kernels.h; bit_block_to_gap, src/bmfunc.h:5542) for block b whose stats are *s: 16-byte
// aligned at g, level bits of gap_calc_level, 0xFFFF padding; *d = its descriptor.  (k_emit_blocks keeps its own copy: calling
// this one from it moved its register allocation.)
// the header, the closing run end, the padding and the descriptor of a GAP block of len runs whose run ends are in g[1 .. len - 1]
__device__ __forceinline__ void gap_close(u16* g, u32 len, u32 first, u64* d, u32 lane)
{
    if (lane == 0) {
        const u32 level = len <= 124u ? 0u : len <= 252u ? 1u : len <= 508u ? 2u : 3u;   // gap_calc_level src/bmfunc.h:5418
        g[0] = (u16)((len << 3) | (level << 1) | first);
        g[len] = 65535u;
        *d = DESC_MAKE_GAP(g, len, first);
    }
    if (lane >= 1u && lane <= 7u && len + lane < ((len + 1u + 7u) & ~7u)) g[len + lane] = 0xFFFFu;
}

__device__ __forceinline__ void gap_write_from_blk(const Blk& b, const BlockStat* s, u16* g, u64* d, u32 lane)
{
    Blk t;
    (void)blk_transitions(b, t, lane);
    const u32 len = uniform32(s->runs);
    u32 idx_base = 1u;                  // first run-end slot
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 c = __popc(t.r[i].x) + __popc(t.r[i].y) + __popc(t.r[i].z) + __popc(t.r[i].w);
        const u32 incl = wave_scan_incl(c, lane);
        u32 idx = idx_base + incl - c;
        const u32 wbase = (u32)i * 256u + lane * 4u;
        const u32 tw[4] = {t.r[i].x, t.r[i].y, t.r[i].z, t.r[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u32 m = tw[j];
            while (m) {
                const u32 k = __builtin_ctz(m); m &= m - 1u;
                g[idx++] = (u16)((wbase + j) * 32u + k - 1u);
            }
        }
        idx_base += __shfl(incl, 63, 64);
    }
    gap_close(g, len, s->first, d, lane);
}

// the 8 KiB image of one touched block in this wave's LDS: its ids [beg, end) ORed in (loads issued 8 per lane at a time)
template <class T>
__device__ __forceinline__ void ids_image(const T* __restrict__ src, u32 beg, u32 end, u32* lds, Blk& b, u32 lane)
{
    u32x4* l4 = reinterpret_cast<u32x4*>(lds);
#pragma unroll
    for (int i = 0; i < 8; ++i) l4[i * 64 + lane] = (u32x4)(0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (u32 k0 = beg; k0 < end; k0 += 512u) {
        u32 o[8];
#pragma unroll
        for (u32 j = 0; j < 8; ++j) { const u32 k = k0 + j * 64u + lane; o[j] = k < end ? id_off(src[k]) : 0xFFFFFFFFu; }
#pragma unroll
        for (u32 j = 0; j < 8; ++j)
            if (o[j] != 0xFFFFFFFFu) atomicOr(&lds[o[j] >> 5], 1u << (o[j] & 31u));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    blk_from_lds(b, lds, lane);
}

// step 5: entry t of the touched-block list (t < totals[1]; entries past it, and blocks outside [blk0, blk0 + nbl), are NULL
// and take no storage).  A touched block is never empty: one run means FULL
template <class T>
__global__ __launch_bounds__(256)
void k_ids_stats(const T* __restrict__ src, const u32* __restrict__ tblk, const u32* __restrict__ tbeg,
                 const u32* __restrict__ totals, u32 cap, u32 blk0, u32 nbl, int optimize, BlockStat* __restrict__ st)
{
    __shared__ u32x4 img[4][512];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 t = uniform32(blockIdx.x * 4u + w);
    if (t >= cap) return;
    const u32 ntouched = uniform32(totals[1]);
    const u32 b = t < ntouched ? uniform32(tblk[t]) : 0xFFFFFFFFu;
    if (b < blk0 || b - blk0 >= nbl) { if (lane == 0) st[t] = BlockStat{0u, 0u, 0u, (u32)K_NULL}; return; }
    if (!optimize) { if (lane == 0) st[t] = BlockStat{0u, 0u, 0u, (u32)K_BIT}; return; }   // (import_block: a bit-block each)
    Blk bb, tr;
    ids_image(src, uniform32(tbeg[t]), uniform32(tbeg[t + 1]), reinterpret_cast<u32*>(img[w]), bb, lane);
    const u32 pop = wave_sum(blk_lane_popcount(bb));
    const u32 runs = 1u + wave_sum(blk_transitions(bb, tr, lane));
    const u32 first = __shfl(bb.r[0].x, 0, 64) & 1u;
    if (lane == 0) st[t] = BlockStat{pop, runs, first, runs == 1u ? (u32)K_FULL : (runs < 1276u ? (u32)K_GAP : (u32)K_BIT)};
}

// step 7: the touched blocks in their final form + their descriptors (desc[] holds NULL everywhere before)
template <class T>
__global__ __launch_bounds__(256)
void k_ids_emit(const T* __restrict__ src, const u32* __restrict__ tblk, const u32* __restrict__ tbeg,
                const u32* __restrict__ totals, u32 cap, u32 blk0, u32 nbl, const BlockStat* __restrict__ st,
                const u32* __restrict__ offs, uint4* __restrict__ bit_slab, u16* __restrict__ gap_slab, u64* __restrict__ desc)
{
    __shared__ u32x4 img[4][512];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 t = uniform32(blockIdx.x * 4u + w);
    if (t >= cap || t >= uniform32(totals[1])) return;
    const u32 b = uniform32(tblk[t]);
    if (b < blk0 || b - blk0 >= nbl) return;
    const u32 nb = b - blk0, kind = uniform32(st[t].kind);
    if (kind == K_FULL) { if (lane == 0) desc[nb] = DESC_MAKE(0, K_FULL); return; }
    Blk bb;
    ids_image(src, uniform32(tbeg[t]), uniform32(tbeg[t + 1]), reinterpret_cast<u32*>(img[w]), bb, lane);
    if (kind == K_BIT) {
        uint4* dst = bit_slab + (size_t)offs[t] * 512u;
        blk_store(bb, as_g4(dst), lane);
        if (lane == 0) desc[nb] = DESC_MAKE(dst, K_BIT);
        return;
    }
    gap_write_from_blk(bb, st + t, gap_slab + offs[t], desc + nb, lane);
}
