// bmx_kernels14.h -- device intervals: a vector from a list of inclusive [left, right] pairs (bvector::set_range src/bm.h:2398 for
// every pair on an empty vector, then optimize()), and a vector as the list of its maximal runs of ones (what a
// bm::interval_enumerator<BV> loop yields, src/bmintervals.h:52-226).  gfx950, wave64.
//
// from_ranges.  Nothing here scales with the covered bits: memory follows the pairs and the blocks of the vector.
//   1. k_rng_scan (+ k_ids_reduce, bmx_kernels13.h)   one pass over the pairs: largest end, "sorted and separated"
//      (l[i] >= r[i-1] + 2 for every i) -- checked, never trusted
//   sorted and separated: the pairs clipped to a block ARE its runs
//   2. k_rng_stats_sorted   one wave per block: two binary searches give the pairs that reach it; runs / first bit / kind from the
//                           pair ends.  No image.
//   4. k_rng_emit_sorted    GAP words straight from the pair ends; only a block of >= 1,276 runs builds an LDS image
//   any other list: no global sort
//   2'. k_rng_count         per pair: <= 2 partial-block pieces counted per block, the whole blocks between them into a
//                           difference array (+1 / -1)
//       k_rs_scan (x2)      bucket ends; blocks covered by a span
//   3'. k_rng_scatter       the pieces (lo | hi << 16) into their block's bucket
//   2". k_rng_stats_any     covered -> FULL, no piece -> NULL, else the pieces ORed into an LDS image and classified
//   4'. k_rng_emit_any      the image rebuilt, written as k_ids_emit writes it
//   3.  k_scan_layout (bmx_kernels.h) between stats and emit, over the blocks in block order in both paths: the table does not
//       depend on the order of the pairs.
// to_ranges.  A start is a one whose predecessor is zero, an end a one whose successor is zero; the k-th start and the k-th end
// belong to the same interval.
//   k_rng_ends_count   starts and ends per block; the neighbour bit across a block border comes from the neighbour's descriptor.
//                      GAP: from the header alone; FULL / NULL: the descriptor
//   k_rs_scan (x2)     running counts
//   k_rng_expand       one wave per block writes its starts to out[2k] and its ends to out[2k + 1]; GAP blocks walk their runs
#pragma once
#include "bmx_kernels13.h"

#define RNG_CHUNK 4096u          // pairs per workgroup of k_rng_scan (256 threads x 16)

template <class T>
__device__ __forceinline__ void rng_pair(const T* __restrict__ p, u64 i, u64& l, u64& r)
{
    const u64 a = (u64)p[2u * i], b = (u64)p[2u * i + 1u];
    l = a < b ? a : b; r = a < b ? b : a;                       // set_range swaps (src/bm.h:2407)
}

// step 1: per chunk its largest end and, in bit 31 of flags[c], whether a pair starts less than 2 past its predecessor's end
// (the format k_ids_reduce folds: info[0] = largest end, info[1] = 1 where the list is not sorted and separated)
template <class T>
__global__ __launch_bounds__(256)
void k_rng_scan(const T* __restrict__ pairs, u64 n, u32* __restrict__ flags, u64* __restrict__ cmax)
{
    __shared__ u64 smx[4];
    __shared__ u32 sfl[4];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u64 base = (u64)blockIdx.x * RNG_CHUNK;
    u64 mx = 0; u32 bad = 0;
#pragma unroll 4
    for (u32 k = 0; k < RNG_CHUNK / 256u; ++k) {
        const u64 i = base + k * 256u + tid;
        if (i < n) {
            u64 l, r; rng_pair(pairs, i, l, r);
            mx = r > mx ? r : mx;
            if (i) { u64 pl, pr; rng_pair(pairs, i - 1u, pl, pr); bad |= (l <= pr) || (l - pr < 2u); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { u64 x = __shfl_xor(mx, o, 64); mx = x > mx ? x : mx; }
    const bool any_bad = __ballot(bad != 0u) != 0ull;
    if (lane == 0) { smx[w] = mx; sfl[w] = any_bad; }
    __syncthreads();
    if (tid == 0) {
        u64 m = smx[0]; u32 f = 0;
#pragma unroll
        for (u32 j = 0; j < 4; ++j) { m = smx[j] > m ? smx[j] : m; f |= sfl[j]; }
        cmax[blockIdx.x] = m; flags[blockIdx.x] = f ? 0x80000000u : 0u;
    }
}

// the 8 KiB image of one block in this wave's LDS: cnt pieces [lo, hi] (in-block, inclusive) ORed in.  Edge words by LDS atomics,
// the words between them by plain stores of all-ones (every writer of a word stores the same value)
template <class S>
__device__ __forceinline__ void rng_image(const S& src, u32 cnt, u32* lds, Blk& b, u32 lane)
{
    u32x4* l4 = reinterpret_cast<u32x4*>(lds);
#pragma unroll
    for (int i = 0; i < 8; ++i) l4[i * 64 + lane] = (u32x4)(0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (u32 k = lane; k < cnt; k += 64u) {
        u32 lo, hi; src.get(k, lo, hi);
        lds_apply_run_edges<GAP_OR>(lds, lo, hi);
        for (u32 wd = (lo >> 5) + 1u; wd < (hi >> 5); ++wd) lds[wd] = ~0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    blk_from_lds(b, lds, lane);
}

// pieces of block (base >> 16) on the sorted path: pairs [p0, p0 + cnt) clipped to it
template <class T>
struct RngSrcPairs {
    const T* __restrict__ pairs; u64 p0, base;
    __device__ __forceinline__ void get(u32 k, u32& lo, u32& hi) const
    {
        u64 l, r; rng_pair(pairs, p0 + k, l, r);
        lo = l < base ? 0u : (u32)(l - base);
        hi = r > base + 65535u ? 65535u : (u32)(r - base);
    }
};
// ... on the bucket path: bucket[beg, beg + cnt)
struct RngSrcBucket {
    const u32* __restrict__ bucket; u32 beg;
    __device__ __forceinline__ void get(u32 k, u32& lo, u32& hi) const { const u32 v = bucket[beg + k]; lo = v & 0xFFFFu; hi = v >> 16; }
};

// step 2 (sorted and separated): block b of the shard [blk0, blk0 + nbl).  Ends ascend, so the first pair with r >= the block's
// first bit and the first pair with l > its last bit bound the pairs that reach it.  runs = 1 + the run ends the pairs give
// (lo - 1 where lo > 0, hi where hi < 65,535)
template <class T>
__global__ __launch_bounds__(256)
void k_rng_stats_sorted(const T* __restrict__ pairs, u64 n, u32 blk0, u32 nbl, BlockStat* __restrict__ st,
                        u32* __restrict__ pfirst, u32* __restrict__ pcnt)
{
    const u32 lane = lane_id();
    const u32 b = uniform32(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= nbl) return;
    const u64 base = ((u64)blk0 + b) << 16, last = base + 65535u;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        u64 l, r; rng_pair(pairs, mid, l, r);
        if (r < base) lo = mid + 1u; else hi = mid;
    }
    const u64 p0 = lo;
    hi = n - p0 > 32769u ? p0 + 32769u : n;                    // (separated pairs: at most 32,768 start in one block, one reaches in)
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        u64 l, r; rng_pair(pairs, mid, l, r);
        if (l <= last) lo = mid + 1u; else hi = mid;
    }
    const u32 cnt = (u32)(lo - p0);
    const RngSrcPairs<T> src{pairs, p0, base};
    u32 words = 0, pop = 0, first = 0;
    for (u32 k = lane; k < cnt; k += 64u) {
        u32 plo, phi; src.get(k, plo, phi);
        words += (plo > 0u) + (phi < 65535u);
        pop += phi - plo + 1u;
        if (k == 0u) first = plo == 0u;
    }
    words = wave_sum(words); pop = wave_sum(pop);
    first = __shfl(first, 0, 64);
    if (lane == 0) {
        const u32 runs = 1u + words;
        const u32 kind = !cnt ? (u32)K_NULL : (runs == 1u ? (u32)K_FULL : (runs < 1276u ? (u32)K_GAP : (u32)K_BIT));
        st[b] = BlockStat{pop, runs, first, kind};
        pfirst[b] = (u32)p0; pcnt[b] = cnt;
    }
}

// step 4 (sorted and separated).  Pair k of a GAP block writes its run ends at slot 1 + 2k, one earlier when the block starts
// with a one (only the first pair can have lo == 0, only the last hi == 65,535)
template <class T>
__global__ __launch_bounds__(256)
void k_rng_emit_sorted(const T* __restrict__ pairs, u32 blk0, u32 nbl, const BlockStat* __restrict__ st,
                       const u32* __restrict__ offs, const u32* __restrict__ pfirst, const u32* __restrict__ pcnt,
                       uint4* __restrict__ bit_slab, u16* __restrict__ gap_slab, u64* __restrict__ desc)
{
    __shared__ u32x4 img[4][512];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= nbl) return;
    const u32 kind = uniform32(st[b].kind);
    if (kind == K_NULL || kind == K_FULL) { if (lane == 0) desc[b] = DESC_MAKE(0, kind); return; }
    const u32 cnt = uniform32(pcnt[b]);
    const RngSrcPairs<T> src{pairs, (u64)uniform32(pfirst[b]), ((u64)blk0 + b) << 16};
    if (kind == K_BIT) {
        Blk bb;
        rng_image(src, cnt, reinterpret_cast<u32*>(img[w]), bb, lane);
        uint4* dst = bit_slab + (size_t)offs[b] * 512u;
        blk_store(bb, as_g4(dst), lane);
        if (lane == 0) desc[b] = DESC_MAKE(dst, K_BIT);
        return;
    }
    u16* g = gap_slab + offs[b];
    const u32 len = uniform32(st[b].runs), first = uniform32(st[b].first);
    for (u32 k = lane; k < cnt; k += 64u) {
        u32 lo, hi; src.get(k, lo, hi);
        u32 idx = 1u + 2u * k - ((first && k) ? 1u : 0u);
        if (lo > 0u) g[idx++] = (u16)(lo - 1u);
        if (hi < 65535u) g[idx] = (u16)hi;
    }
    gap_close(g, len, first, desc + b, lane);
}

// the pieces of pair [l, r] inside the shard [B0, B0 + nbl): f(block - B0, lo, hi) for the (at most two) blocks the pair covers
// partly or alone; the whole blocks between them are the span [s0, s1] (s0 > s1: none)
template <class F>
__device__ __forceinline__ void rng_pieces(u64 l, u64 r, u64 B0, u64 nbl, u64& s0, u64& s1, F f)
{
    const u64 bl = l >> 16, br = r >> 16, B1 = B0 + nbl;
    s0 = 1; s1 = 0;
    if (br < B0 || bl >= B1) return;
    if (bl == br) { f((u32)(bl - B0), (u32)l & 0xFFFFu, (u32)r & 0xFFFFu); return; }
    if (bl >= B0) f((u32)(bl - B0), (u32)l & 0xFFFFu, 65535u);
    if (br < B1) f((u32)(br - B0), 0u, (u32)r & 0xFFFFu);
    s0 = bl + 1u > B0 ? bl + 1u : B0;
    s1 = br - 1u < B1 - 1u ? br - 1u : B1 - 1u;
}

// step 2' (any list).  cnt: nbl entries, diff: nbl + 1 entries, both zero before
template <class T>
__global__ __launch_bounds__(256)
void k_rng_count(const T* __restrict__ pairs, u64 n, u32 blk0, u32 nbl, u32* __restrict__ cnt, u32* __restrict__ diff)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        u64 l, r, s0, s1; rng_pair(pairs, i, l, r);
        rng_pieces(l, r, (u64)blk0, (u64)nbl, s0, s1, [&](u32 b, u32, u32) { atomicAdd(&cnt[b], 1u); });
        if (s0 <= s1) { atomicAdd(&diff[s0 - blk0], 1u); atomicAdd(&diff[s1 + 1u - blk0], 0xFFFFFFFFu); }
    }
}

// step 3': bucket of block b = bucket[pend[b] - count(b), pend[b]) (pend: inclusive running count); cnt[] counts down to zero
template <class T>
__global__ __launch_bounds__(256)
void k_rng_scatter(const T* __restrict__ pairs, u64 n, u32 blk0, u32 nbl, const u64* __restrict__ pend, u32* __restrict__ cnt,
                   u32* __restrict__ bucket)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        u64 l, r, s0, s1; rng_pair(pairs, i, l, r);
        rng_pieces(l, r, (u64)blk0, (u64)nbl, s0, s1, [&](u32 b, u32 lo, u32 hi) {
            const u32 left = atomicSub(&cnt[b], 1u);               // (count(b) .. 1)
            bucket[(u32)pend[b] - left] = lo | (hi << 16);
        });
    }
}

// step 2" (any list): cover = inclusive running sum of the difference array (low 32 bits: sums are taken mod 2^32 and a block is
// covered by fewer than 2^32 pairs)
__global__ __launch_bounds__(256)
void k_rng_stats_any(const u32* __restrict__ bucket, const u64* __restrict__ pend, const u64* __restrict__ cover, u32 nbl,
                     BlockStat* __restrict__ st)
{
    __shared__ u32x4 img[4][512];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= nbl) return;
    if (uniform32((u32)cover[b]) != 0u) { if (lane == 0) st[b] = BlockStat{65536u, 1u, 1u, (u32)K_FULL}; return; }
    const u32 beg = b ? uniform32((u32)pend[b - 1u]) : 0u, end = uniform32((u32)pend[b]);
    if (beg == end) { if (lane == 0) st[b] = BlockStat{0u, 0u, 0u, (u32)K_NULL}; return; }
    Blk bb, tr;
    rng_image(RngSrcBucket{bucket, beg}, end - beg, reinterpret_cast<u32*>(img[w]), bb, lane);
    const u32 pop = wave_sum(blk_lane_popcount(bb));
    const u32 runs = 1u + wave_sum(blk_transitions(bb, tr, lane));
    const u32 first = __shfl(bb.r[0].x, 0, 64) & 1u;
    if (lane == 0) st[b] = BlockStat{pop, runs, first, runs == 1u ? (u32)K_FULL : (runs < 1276u ? (u32)K_GAP : (u32)K_BIT)};
}

// step 4' (any list)
__global__ __launch_bounds__(256)
void k_rng_emit_any(const u32* __restrict__ bucket, const u64* __restrict__ pend, u32 nbl, const BlockStat* __restrict__ st,
                    const u32* __restrict__ offs, uint4* __restrict__ bit_slab, u16* __restrict__ gap_slab, u64* __restrict__ desc)
{
    __shared__ u32x4 img[4][512];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= nbl) return;
    const u32 kind = uniform32(st[b].kind);
    if (kind == K_NULL || kind == K_FULL) { if (lane == 0) desc[b] = DESC_MAKE(0, kind); return; }
    const u32 beg = b ? uniform32((u32)pend[b - 1u]) : 0u, end = uniform32((u32)pend[b]);
    Blk bb;
    rng_image(RngSrcBucket{bucket, beg}, end - beg, reinterpret_cast<u32*>(img[w]), bb, lane);
    if (kind == K_BIT) {
        uint4* dst = bit_slab + (size_t)offs[b] * 512u;
        blk_store(bb, as_g4(dst), lane);
        if (lane == 0) desc[b] = DESC_MAKE(dst, K_BIT);
        return;
    }
    gap_write_from_blk(bb, st + b, gap_slab + offs[b], desc + b, lane);
}

// ---------------------------------------------------------------------------
// to_ranges
// ---------------------------------------------------------------------------
// first / last bit of a block from its descriptor: NULL 0, FULL 1, bit-block word 0 bit 0 / word 2047 bit 31, GAP the header's
// start bit / the value of its last run (runs alternate)
__device__ __forceinline__ u32 desc_first_bit(u64 d)
{
    const u32 k = DESC_K(d);
    if (k == K_BIT) return *reinterpret_cast<const u32*>((uintptr_t)DESC_P(d)) & 1u;
    return k == K_GAP ? (GMETA(d) & 1u) : (k == K_FULL ? 1u : 0u);
}
__device__ __forceinline__ u32 desc_last_bit(u64 d)
{
    const u32 k = DESC_K(d);
    if (k == K_BIT) return reinterpret_cast<const u32*>((uintptr_t)DESC_P(d))[2047] >> 31;
    return k == K_GAP ? ((GMETA(d) ^ ((GMETA(d) >> 1) - 1u)) & 1u) : (k == K_FULL ? 1u : 0u);
}

// per block its starts (ones whose predecessor is zero) and ends (ones whose successor is zero).  A GAP block is counted from its
// header: its runs of ones, less the first one where the previous block ends with a one, less the last one where the next block
// starts with a one.  Bit-block: S = transitions & x, E = transitions & ~x (a zero that differs from its predecessor: the end is
// the bit before), plus the block's own first / last bit
__global__ __launch_bounds__(256)
void k_rng_ends_count(const u64* __restrict__ desc, u32 nblocks, u32* __restrict__ cs, u32* __restrict__ ce)
{
    const u32 lane = lane_id();
    const u32 nb = uniform32(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (nb >= nblocks) return;
    const u64 d = uniform64(desc[nb]);
    const u32 k = DESC_K(d);
    u32 s = 0, e = 0;
    if (k != K_NULL) {
        const u32 prev = nb ? uniform32(desc_last_bit(uniform64(desc[nb - 1u]))) : 0u;
        const u32 next = nb + 1u < nblocks ? uniform32(desc_first_bit(uniform64(desc[nb + 1u]))) : 0u;
        if (k == K_FULL) { s = !prev; e = !next; }
        else if (k == K_GAP) {
            const u32 len = GMETA(d) >> 1, sbit = GMETA(d) & 1u, lbit = (sbit ^ (len - 1u)) & 1u;
            const u32 ones = sbit ? (len + 1u) >> 1 : len >> 1;
            s = ones - (sbit & prev); e = ones - (lbit & next);
        } else {
            Blk b, t;
            blk_load(b, as_gc4(DESC_P(d)), lane);
            (void)blk_transitions(b, t, lane);
            u32 ls = 0, le = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ls += __popc(t.r[i].x & b.r[i].x) + __popc(t.r[i].y & b.r[i].y) + __popc(t.r[i].z & b.r[i].z) + __popc(t.r[i].w & b.r[i].w);
                le += __popc(t.r[i].x & ~b.r[i].x) + __popc(t.r[i].y & ~b.r[i].y) + __popc(t.r[i].z & ~b.r[i].z) + __popc(t.r[i].w & ~b.r[i].w);
            }
            const u32 fbit = __shfl(b.r[0].x, 0, 64) & 1u, lbit = __shfl(b.r[7].w, 63, 64) >> 31;
            s = wave_sum(ls) + (fbit & (prev ^ 1u)); e = wave_sum(le) + (lbit & (next ^ 1u));
        }
    }
    if (lane == 0) { cs[nb] = s; ce[nb] = e; }
}

// the set bits of w as out[2 * (off++) + which] = base + bit - which   (which = 0: starts; 1: ends, marked one bit late)
template <typename T>
__device__ __forceinline__ void rng_emit_word(u32 w, u64 base, u32 which, T* __restrict__ out, u64& off)
{
    while (w) { const u32 b = (u32)__builtin_ctz(w); out[2u * (off++) + which] = (T)(base + b - which); w &= w - 1u; }
}

// rs / re: inclusive running counts of starts / ends per block; the call has checked that the total fits the buffer
template <typename T>
__global__ __launch_bounds__(256)
void k_rng_expand(const u64* __restrict__ desc, u32 nblocks, const u64* __restrict__ rs, const u64* __restrict__ re,
                  T* __restrict__ out, u64 cap)
{
    const u32 lane = lane_id();
    const u32 nb = uniform32(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (nb >= nblocks) return;
    const u64 d = uniform64(desc[nb]);
    const u32 k = DESC_K(d);
    if (k == K_NULL) return;
    const u64 s0 = nb ? rs[nb - 1u] : 0ull, e0 = nb ? re[nb - 1u] : 0ull;
    const u64 s1 = rs[nb], e1 = re[nb];
    if (s1 > cap || e1 > cap) return;                           // (never reached: the call fails with the needed size)
    const u32 prev = nb ? uniform32(desc_last_bit(uniform64(desc[nb - 1u]))) : 0u;
    const u32 next = nb + 1u < nblocks ? uniform32(desc_first_bit(uniform64(desc[nb + 1u]))) : 0u;
    const u64 bit0 = (u64)nb << 16;
    if (k == K_FULL) {
        if (lane == 0) { if (!prev) out[2u * s0] = (T)bit0; if (!next) out[2u * e0 + 1u] = (T)(bit0 + 65535u); }
        return;
    }
    if (k == K_GAP) {
        const gcptr16 g = as_gc16(DESC_P(d));
        const u32 len = GMETA(d) >> 1, sbit = GMETA(d) & 1u;
        const u32 ones = sbit ? (len + 1u) >> 1 : len >> 1;
        const u32 skip = sbit & prev;                           // the block's first one continues the previous block's run
        for (u32 j = lane; j < ones; j += 64u) {
            const u32 r = 2u * j + (sbit ^ 1u);                 // run r covers (g[r], g[r + 1]], run 0 from bit 0
            if (!(r == 0u && skip)) out[2u * (s0 + j - skip)] = (T)(bit0 + (r ? (u32)g[r] + 1u : 0u));
            if (!(r == len - 1u && next)) out[2u * (e0 + j) + 1u] = (T)(bit0 + (u32)g[r + 1u]);
        }
        return;
    }
    Blk b, t;
    blk_load(b, as_gc4(DESC_P(d)), lane);
    (void)blk_transitions(b, t, lane);
    const u32 fbit = __shfl(b.r[0].x, 0, 64) & 1u, lbit = __shfl(b.r[7].w, 63, 64) >> 31;
    u64 srow = s0, erow = e0;
    if (fbit & (prev ^ 1u)) { if (lane == 0) out[2u * s0] = (T)bit0; ++srow; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 x[4] = {b.r[i].x, b.r[i].y, b.r[i].z, b.r[i].w}, tw[4] = {t.r[i].x, t.r[i].y, t.r[i].z, t.r[i].w};
        u32 c_s = 0, c_e = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c_s += __popc(tw[j] & x[j]); c_e += __popc(tw[j] & ~x[j]); }
        const u32 is = wave_scan_incl(c_s, lane), ie = wave_scan_incl(c_e, lane);
        u64 so = srow + (is - c_s), eo = erow + (ie - c_e);
        const u64 wb = bit0 + ((u64)((u32)i * 256u + lane * 4u) << 5);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rng_emit_word<T>(tw[j] & x[j], wb + 32u * (u32)j, 0u, out, so);
            rng_emit_word<T>(tw[j] & ~x[j], wb + 32u * (u32)j, 1u, out, eo);
        }
        srow += uniform32(__shfl(is, 63, 64)); erow += uniform32(__shfl(ie, 63, 64));
    }
    if ((lbit & (next ^ 1u)) && lane == 0) out[2u * erow + 1u] = (T)(bit0 + 65535u);
}
