// bmx_kernels15.h -- rank-space translation of whole vectors: bm::rank_compressor (src/bmalgo.h:452-707).  gfx950, wave64.
//
//   compress   (extract): bit r of the target is set iff the r-th one of idx (0-based) is set in src
//   decompress (deposit): bit p of the target is set iff p is a one of idx and bit rank_idx(p) - 1 of src is set
//
// Both need P[b], the ones of idx up to and including block b (the running counts of a rank-select index, or k_block_counts +
// k_rs_scan).  The house pattern of bmx_kernels13.h: a stats pass to BlockStat, k_scan_layout, an emit pass that computes the
// block again and writes it in its final form.  Work items are (source, block) pairs: blockIdx.y is the source of a batch.
//
//   deposit  one wave per block b of idx.  Its ranks [P[b-1], P[b]) are a window of <= 65,536 bits of src that spans at most
//            two src blocks: the window is staged in the wave's 16 KiB of LDS as a bit image, the lanes scan the popcounts of the
//            index words, and index word m at rank offset o takes popc(m) window bits at o (two LDS words, one funnel shift)
//            and deposits them under m.  Every output word is written once, by its own lane.
//   extract  one workgroup per target block t.  Its ones come from the index blocks [b0, b1] found by binary search of
//            t * 65,536 in P; the four waves take those blocks in turn, form src & idx, extract every word under its index word
//            and OR the packed bits into the workgroup's LDS image at P[b-1] + in-block prefix - t * 65,536 (LDS atomicOr:
//            a word touches at most two target words; what falls outside the image belongs to a neighbour, who clips it too).
//   positions  for sparse operands: the ranks of src & idx (compress: one wave per index block, k_rankc_cpos) or the positions of
//            the deposited block (decompress, k_rankc_dpos) as an ascending list, handed to the sorted path of from_indices.
//
// CDNA has no bit extract / deposit under a mask: word_extract / word_deposit below are a loop over the set bits for sparse
// words and a five-step log network for dense ones, chosen per 256-word row of a wave (no lane then waits for another's loop).
#pragma once
#include "bmx_kernels14.h"

struct RankcSrc { const u64* desc; u32 nblocks; u32 pad; };              // a source's table; desc == null: no such plane
struct RankcOut { uint4* bits; u16* gaps; u64* desc; u64 pad; };         // a target's slabs and table

// ---- one 32-bit word ------------------------------------------------------------------------------------------------------
// the moves of the log network for mask m: mv[i] = the mask bits that step i moves by 2^i.  With mk = the zeros of m shifted up,
// the prefix-XOR of mk marks the bits with an odd number of zeros below them
__device__ __forceinline__ void word_moves(u32 m, u32 mv[5])
{
    u32 mk = ~m << 1;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const u32 mp = prefix_xor32(mk);
        mv[i] = mp & m;
        m = (m ^ mv[i]) | (mv[i] >> (1u << i));
        mk &= ~mp;
    }
}
// the bits of x under m, packed to the low end
__device__ __forceinline__ u32 word_extract_net(u32 x, u32 m)
{
    u32 mv[5]; word_moves(m, mv);
    x &= m;
#pragma unroll
    for (int i = 0; i < 5; ++i) { const u32 t = x & mv[i]; x = (x ^ t) | (t >> (1u << i)); }
    return x;
}
// the low popc(m) bits of x, spread to the set bits of m
__device__ __forceinline__ u32 word_deposit_net(u32 x, u32 m)
{
    u32 mv[5]; word_moves(m, mv);
#pragma unroll
    for (int i = 4; i >= 0; --i) { const u32 t = x << (1u << i); x = (x & ~mv[i]) | (t & mv[i]); }
    return x & m;
}
// x must be a subset of m: a step per set bit of x
__device__ __forceinline__ u32 word_extract_loop(u32 x, u32 m)
{
    u32 r = 0;
    while (x) { const u32 p = (u32)__builtin_ctz(x); x &= x - 1u; r |= 1u << __popc(m & ((1u << p) - 1u)); }
    return r;
}
// a step per set bit of m
__device__ __forceinline__ u32 word_deposit_loop(u32 x, u32 m)
{
    u32 r = 0;
    while (m) { const u32 low = m & (0u - m); r |= (x & 1u) ? low : 0u; x >>= 1; m ^= low; }
    return r;
}
__device__ __forceinline__ u32 word_extract(u32 x, u32 m, bool net)
{
    x &= m;
    if (!x) return 0u;
    if (m == ~0u) return x;
    return net ? word_extract_net(x, m) : word_extract_loop(x, m);
}
__device__ __forceinline__ u32 word_deposit(u32 x, u32 m, bool net)
{
    if (m == ~0u) return x;
    return net ? word_deposit_net(x, m) : word_deposit_loop(x, m);
}
#define RANKC_NET_ROW 1536u     // a row of 256 words goes through the network from 6 bits per word on average

__device__ __forceinline__ u32 row_popc(const u32x4& r) { return (u32)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w)); }

// ---- deposit --------------------------------------------------------------------------------------------------------------
// 32 bits of the window image from bit o on (o + the bits used stays inside the 4,096 words: the clamp never changes a used bit)
__device__ __forceinline__ u32 window_bits(const u32* win, u32 o)
{
    const u32 wi = o >> 5, wj = wi + 1u < 4096u ? wi + 1u : 4095u;
    return __builtin_amdgcn_alignbit(win[wj], win[wi], o & 31u);
}

// the target block b of source s into out; false: the block receives no bit (NULL).  lds: 4,096 words of this wave
__device__ __forceinline__ bool rankc_deposit_block(const u64* __restrict__ idesc, const u64* __restrict__ P, u32 b,
                                                    const RankcSrc s, u32* lds, Blk& out, u32 lane)
{
    const u64 d = uniform64(idesc[b]);
    if (DESC_K(d) == K_NULL) return false;
    const u64 r0 = b ? uniform64(P[b - 1u]) : 0ull, r1 = uniform64(P[b]);
    if (r1 == r0) return false;
    const u32 sb0 = (u32)(r0 >> 16), sb1 = (u32)((r1 - 1ull) >> 16);
    const u64 d0 = sb0 < s.nblocks ? uniform64(s.desc[sb0]) : 0ull;
    const u64 d1 = (sb1 != sb0 && sb1 < s.nblocks) ? uniform64(s.desc[sb1]) : 0ull;
    if (DESC_K(d0) == K_NULL && DESC_K(d1) == K_NULL) return false;            // window all NULL: the index block is not read
    Blk m;
    blk_from_desc(d, m, lds, lane);
    if (DESC_K(d0) == K_FULL && (sb1 == sb0 || DESC_K(d1) == K_FULL)) { out = m; return true; }   // window all FULL: the index block
    {
        Blk t;
        blk_from_desc(d0, t, lds, lane);
        blk_to_lds(t, lds, lane);
        blk_from_desc(d1, t, lds + 2048, lane);
        blk_to_lds(t, lds + 2048, lane);
    }
    u32 row_base = (u32)r0 & 0xFFFFu;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 c = row_popc(m.r[i]);
        const u32 incl = wave_scan_incl(c, lane);
        const u32 tot = uniform32(__shfl(incl, 63, 64));
        const bool net = tot >= RANKC_NET_ROW;
        u32 o = row_base + incl - c;
        const u32 mw[4] = {m.r[i].x, m.r[i].y, m.r[i].z, m.r[i].w};
        u32 ow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ow[j] = mw[j] ? word_deposit(window_bits(lds, o), mw[j], net) : 0u;
            o += (u32)__popc(mw[j]);
        }
        out.r[i].x = ow[0]; out.r[i].y = ow[1]; out.r[i].z = ow[2]; out.r[i].w = ow[3];
        row_base += tot;
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// the storage decision of a target block: no bit -> NULL; without optimize a bit-block; with it the rule of k_block_stats
__device__ __forceinline__ BlockStat rankc_classify(const Blk& b, int optimize, u32 lane)
{
    Blk tr;
    const u32 pop = wave_sum(blk_lane_popcount(b));
    const u32 runs = 1u + wave_sum(blk_transitions(b, tr, lane));
    const u32 first = __shfl(b.r[0].x, 0, 64) & 1u;
    const u32 kind = !pop ? (u32)K_NULL : !optimize ? (u32)K_BIT : runs == 1u ? (u32)K_FULL : runs < 1276u ? (u32)K_GAP : (u32)K_BIT;
    return BlockStat{pop, runs, first, kind};
}

__device__ __forceinline__ void rankc_write_block(const Blk& bb, const BlockStat* st, u32 off, const RankcOut o, u32 nb, u32 lane)
{
    const u32 kind = uniform32(st->kind);
    if (kind == K_NULL || kind == K_FULL) { if (lane == 0) o.desc[nb] = DESC_MAKE(0, kind); return; }
    if (kind == K_BIT) {
        uint4* dst = o.bits + (size_t)off * 512u;
        blk_store(bb, as_g4(dst), lane);
        if (lane == 0) o.desc[nb] = DESC_MAKE(dst, K_BIT);
        return;
    }
    gap_write_from_blk(bb, st, o.gaps + off, o.desc + nb, lane);
}

// the ascending positions of the ones of bb (bit 0 of the block = bit0) to out[first ..]
__device__ __forceinline__ void blk_emit_positions(const Blk& bb, u64 bit0, u64* __restrict__ out, u64 first, u32 lane)
{
    u64 row_off = first;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 c = row_popc(bb.r[i]);
        const u32 incl = wave_scan_incl(c, lane);
        u64 off = row_off + (incl - c);
        const u64 wb = bit0 + ((u64)((u32)i * 256u + lane * 4u) << 5);
        emit_word_bits<u64>(bb.r[i].x, wb, out, off);
        emit_word_bits<u64>(bb.r[i].y, wb + 32u, out, off);
        emit_word_bits<u64>(bb.r[i].z, wb + 64u, out, off);
        emit_word_bits<u64>(bb.r[i].w, wb + 96u, out, off);
        row_off += uniform32(__shfl(incl, 63, 64));
    }
}

// stats of target block b of source blockIdx.y: st[s * inb + b] and / or its popcount in cnt[s * inb + b]
__global__ __launch_bounds__(256)
void k_rankc_dstats(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, const RankcSrc* __restrict__ srcs,
                    int optimize, BlockStat* __restrict__ st, u32* __restrict__ cnt)
{
    __shared__ u32 lds[4 * 4096];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= inb) return;
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    const size_t e = (size_t)blockIdx.y * inb + b;
    Blk bb;
    BlockStat r = BlockStat{0u, 0u, 0u, (u32)K_NULL};
    if (rankc_deposit_block(idesc, P, b, s, lds + w * 4096u, bb, lane)) r = rankc_classify(bb, optimize, lane);
    if (lane == 0) { if (st) st[e] = r; if (cnt) cnt[e] = r.pop; }
}

__global__ __launch_bounds__(256)
void k_rankc_demit(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, const RankcSrc* __restrict__ srcs,
                   const BlockStat* __restrict__ st, const u32* __restrict__ offs, const RankcOut* __restrict__ outs)
{
    __shared__ u32 lds[4 * 4096];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= inb) return;
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    const RankcOut o = outs[blockIdx.y];
    const size_t e = (size_t)blockIdx.y * inb + b;
    const u32 kind = uniform32(st[e].kind);
    if (kind == K_NULL || kind == K_FULL) { if (lane == 0) o.desc[b] = DESC_MAKE(0, kind); return; }
    Blk bb;
    if (!rankc_deposit_block(idesc, P, b, s, lds + w * 4096u, bb, lane)) return;      // (never: the stats pass saw bits)
    rankc_write_block(bb, st + e, offs[e], o, b, lane);
}

// positions path of decompress: rc = inclusive running popcounts of the target blocks of each source, base[s] = where the
// list of source s starts in out
__global__ __launch_bounds__(256)
void k_rankc_dpos(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, const RankcSrc* __restrict__ srcs,
                  const u64* __restrict__ rc, const u64* __restrict__ base, u64* __restrict__ out)
{
    __shared__ u32 lds[4 * 4096];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= inb) return;
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    const u64* r = rc + (size_t)blockIdx.y * inb;
    const u64 first = b ? uniform64(r[b - 1u]) : 0ull;
    if (uniform64(r[b]) == first) return;
    Blk bb;
    if (!rankc_deposit_block(idesc, P, b, s, lds + w * 4096u, bb, lane)) return;
    blk_emit_positions(bb, (u64)b << 16, out, base[blockIdx.y] + first, lane);
}

// ---- extract --------------------------------------------------------------------------------------------------------------
// the first block whose running count exceeds v (inb where none does)
__device__ __forceinline__ u32 rankc_search(const u64* __restrict__ P, u32 inb, u64 v)
{
    u32 lo = 0, hi = inb;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (P[mid] > v) hi = mid; else lo = mid + 1u; }
    return lo;
}

// src & idx of index block b of source s; false where it is empty (a NULL source block: the index block is not read)
__device__ __forceinline__ bool rankc_and_block(const u64* __restrict__ idesc, u32 b, const RankcSrc s, u32* scr, Blk& m, Blk& a,
                                                u32 lane)
{
    const u64 sd = b < s.nblocks ? uniform64(s.desc[b]) : 0ull;
    if (DESC_K(sd) == K_NULL) return false;
    const u64 d = uniform64(idesc[b]);
    if (DESC_K(d) == K_NULL) return false;
    blk_from_desc(d, m, scr, lane);
    if (DESC_K(sd) == K_FULL) a = m;
    else { blk_from_desc(sd, a, scr, lane); blk_and(a, m); }
    return !blk_is_zero(a);
}

// the image of target block t of source s in img (2,048 words of the workgroup); scr: 4 x 2,048 words.  All 256 threads call
__device__ __forceinline__ void rankc_extract_image(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, u64 total,
                                                    u32 t, const RankcSrc s, u32* img, u32* scr, u32* rng)
{
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u64 lo = (u64)t << 16, hi = lo + 65536ull < total ? lo + 65536ull : total;
    if (threadIdx.x == 0) { rng[0] = rankc_search(P, inb, lo); rng[1] = rankc_search(P, inb, hi - 1ull); }
    for (u32 k = threadIdx.x; k < 2048u; k += 256u) img[k] = 0u;
    __syncthreads();
    const u32 b0 = rng[0], b1 = rng[1] < inb ? rng[1] : inb - 1u;
    for (u32 b = b0 + w; b <= b1; b += 4u) {
        Blk m, a;
        if (!rankc_and_block(idesc, b, s, scr + w * 2048u, m, a, lane)) continue;
        // offset of the block's first one in the image: in (-65,536, 65,536)
        int row_base = (int)(long long)((b ? P[b - 1u] : 0ull) - lo);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u32 c = row_popc(m.r[i]);
            const u32 incl = wave_scan_incl(c, lane);
            const u32 ca = uniform32(wave_sum(row_popc(a.r[i])));
            const bool net = ca >= 1024u;                                           // 4 source bits per word on average
            int o = row_base + (int)(incl - c);
            const u32 mw[4] = {m.r[i].x, m.r[i].y, m.r[i].z, m.r[i].w};
            const u32 aw[4] = {a.r[i].x, a.r[i].y, a.r[i].z, a.r[i].w};
            if (ca) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32 bits = aw[j] ? word_extract(aw[j], mw[j], net) : 0u;
                    if (bits) {
                        const int wi = o >> 5;
                        const u64 v = (u64)bits << ((u32)o & 31u);
                        if ((u32)wi < 2048u && (u32)v) atomicOr(&img[wi], (u32)v);
                        if ((u32)(wi + 1) < 2048u && (u32)(v >> 32)) atomicOr(&img[wi + 1], (u32)(v >> 32));
                    }
                    o += __popc(mw[j]);
                }
            }
            row_base += (int)uniform32(__shfl(incl, 63, 64));
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256)
void k_rankc_cstats(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, u64 total, u32 nbt,
                    const RankcSrc* __restrict__ srcs, int optimize, BlockStat* __restrict__ st)
{
    __shared__ u32 img[2048];
    __shared__ u32 scr[4 * 2048];
    __shared__ u32 rng[2];
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    rankc_extract_image(idesc, inb, P, total, blockIdx.x, s, img, scr, rng);
    if (threadIdx.x >= 64u) return;
    Blk bb;
    blk_from_lds(bb, img, threadIdx.x);
    const BlockStat r = rankc_classify(bb, optimize, threadIdx.x);
    if (threadIdx.x == 0) st[(size_t)blockIdx.y * nbt + blockIdx.x] = r;
}

__global__ __launch_bounds__(256)
void k_rankc_cemit(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, u64 total, u32 nbt,
                   const RankcSrc* __restrict__ srcs, const BlockStat* __restrict__ st, const u32* __restrict__ offs,
                   const RankcOut* __restrict__ outs)
{
    __shared__ u32 img[2048];
    __shared__ u32 scr[4 * 2048];
    __shared__ u32 rng[2];
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    const RankcOut o = outs[blockIdx.y];
    const size_t e = (size_t)blockIdx.y * nbt + blockIdx.x;
    const u32 kind = st[e].kind;                                                    // (workgroup-uniform)
    if (kind == K_NULL || kind == K_FULL) { if (threadIdx.x == 0) o.desc[blockIdx.x] = DESC_MAKE(0, kind); return; }
    rankc_extract_image(idesc, inb, P, total, blockIdx.x, s, img, scr, rng);
    if (threadIdx.x >= 64u) return;
    Blk bb;
    blk_from_lds(bb, img, threadIdx.x);
    rankc_write_block(bb, st + e, offs[e], o, blockIdx.x, threadIdx.x);
}

// positions path of compress, one wave per index block b of source blockIdx.y.  COUNT: cnt[s * inb + b] = the ones of
// src & idx in the block.  Else: their ranks, ascending, to out[base[s] + the ones of src & idx before the block ..]
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_rankc_cpos(const u64* __restrict__ idesc, u32 inb, const u64* __restrict__ P, const RankcSrc* __restrict__ srcs,
                  u32* __restrict__ cnt, const u64* __restrict__ rc, const u64* __restrict__ base, u64* __restrict__ out)
{
    __shared__ u32 scr[4 * 2048];
    const u32 lane = lane_id(), w = threadIdx.x >> 6;
    const u32 b = uniform32(blockIdx.x * 4u + w);
    if (b >= inb) return;
    const RankcSrc s = srcs[blockIdx.y];
    if (!s.desc) return;
    const size_t e = (size_t)blockIdx.y * inb + b;
    if (!COUNT) { const u64 before = b ? rc[e - 1u] : 0ull; if (rc[e] == before) return; }
    Blk m, a;
    const bool any = rankc_and_block(idesc, b, s, scr + w * 2048u, m, a, lane);
    if (COUNT) {
        const u32 c = any ? wave_sum(blk_lane_popcount(a)) : 0u;
        if (lane == 0) cnt[e] = c;
        return;
    }
    if (!any) return;
    u64 rank_base = b ? P[b - 1u] : 0ull;
    u64 out_base = base[blockIdx.y] + (b ? rc[e - 1u] : 0ull);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 cm = row_popc(m.r[i]), ca = row_popc(a.r[i]);
        const u32 im = wave_scan_incl(cm, lane), ia = wave_scan_incl(ca, lane);
        u64 rk = rank_base + (im - cm), off = out_base + (ia - ca);
        const u32 mw[4] = {m.r[i].x, m.r[i].y, m.r[i].z, m.r[i].w};
        const u32 aw[4] = {a.r[i].x, a.r[i].y, a.r[i].z, a.r[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u32 x = aw[j];
            while (x) { const u32 p = (u32)__builtin_ctz(x); x &= x - 1u; out[off++] = rk + (u32)__popc(mw[j] & ((1u << p) - 1u)); }
            rk += (u32)__popc(mw[j]);
        }
        rank_base += uniform32(__shfl(im, 63, 64));
        out_base += uniform32(__shfl(ia, 63, 64));
    }
}
