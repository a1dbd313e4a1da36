// bmx_kernels12.h -- bm::distance_operation (src/bmalgo_impl.h:766) and all-pairs distance matrices (gfx950, wave64).
//
// One pair: |A & B|, |A| and |B| of two vectors in ONE pass over both (the metrics of bmalgo_impl.h:57-66 all follow from
// these three by exact u64 arithmetic on the host).  k_distance_pair_stream is the all-bit-block twin of k_count_op2_stream,
// k_distance_pair_loop the any-kinds twin of k_count_op2_loop; both fold three counts where those fold one.
//
// All pairs: the first GEMM-shaped operation of the library.  A workgroup owns a tile of DM_T A-vectors x DM_T B-vectors
// and a range of block columns; per column it stages the tile's blocks chunk by chunk (DM_K words of every row) into LDS
// and every thread keeps a 4 x 4 register tile of u32 counters updated with AND + popcount-accumulate (v_bcnt_u32_b32).
// Each staged word is read from HBM once per tile and used DM_T times from LDS, so the kernel is VALU-bound where the
// one-pair-at-a-time route is HBM-bound.  Partial tiles are merged into the u64 output with vector u64 atomics.
// The staging reads NULL / FULL / bit-blocks only: GAP blocks are expanded into bit-blocks by k_gap_expand before the
// launch (DESIGN_KERNELS.md 2.18).
#pragma once
#include "bmx_kernels2.h"

// ---- three counts folded by the last workgroup --------------------------------------------------------------------------
// Words 0..2 of each COUNT_SLOTS line of the count fold (the one-count folds use word 0 only; every word is left at zero
// again by the folding wave).  The tickets are fold_publish's: with v = 0 it only draws the workgroup's ticket.
__device__ __forceinline__ void count3_fanin_fold(u32 c0, u32 c1, u32 c2, FoldOut f, u32 lane, u32 wave)
{
    __shared__ u32 part3[16 * 3];
    const u32 nw = blockDim.x >> 6;
    if (lane == 0) { part3[wave * 3u] = c0; part3[wave * 3u + 1u] = c1; part3[wave * 3u + 2u] = c2; }
    __syncthreads();
    if (wave == 0) {
        u32 folder = 0;
        if (lane == 0) {
            u64 t0 = 0, t1 = 0, t2 = 0;
            for (u32 i = 0; i < nw; ++i) { t0 += part3[i * 3u]; t1 += part3[i * 3u + 1u]; t2 += part3[i * 3u + 2u]; }
            u64* slot = f.slots + (blockIdx.x % COUNT_SLOTS) * COUNT_SLOT_STRIDE;
            if (t0) (void)__hip_atomic_fetch_add(slot, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t1) (void)__hip_atomic_fetch_add(slot + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t2) (void)__hip_atomic_fetch_add(slot + 2, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the adds have been performed before the ticket is drawn
            folder = fold_publish(0ull, f) ? 1u : 0u;
        }
        if (__shfl(folder, 0, 64)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u64 v = __hip_atomic_exchange(f.slots + lane * COUNT_SLOT_STRIDE + k, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) __hip_atomic_store(f.out + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// |A & B|, |A|, |B| of one register-image column pair, lane-local
__device__ __forceinline__ void dist_eat(Blk& x, const Blk& y, u32& cab, u32& ca, u32& cb)
{
    ca += blk_lane_popcount(x);
    cb += blk_lane_popcount(y);
    blk_and(x, y);
    cab += blk_lane_popcount(x);
}

// both operands bit-blocks only, same length: a wave streams a contiguous stretch of columns, two in flight
// (the load schedule of k_count_op2_stream)
template <int WAVES, bool NT>
__global__ __launch_bounds__(WAVES * 64)
void k_distance_pair_stream(const u64* __restrict__ da, const u64* __restrict__ db, u32 nblocks, u32 per_wave, FoldOut fold)
{
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 w = uniform32(blockIdx.x * (u32)WAVES + wave);
    const u32 c0 = w * per_wave;
    const u32 c1 = c0 + per_wave < nblocks ? c0 + per_wave : nblocks;
    u32 cab = 0, ca = 0, cb = 0;
    if (c0 < c1) {
        const u32 last = nblocks - 1u;
        auto ptr = [&](const u64* __restrict__ d, u32 c) { return DESC_P(uniform64(d[c < last ? c : last])); };
        auto load = [&](Blk& x, Blk& y, u64 pa, u64 pb) { part_load<8, NT>(x, as_gc4(pa), lane); part_load<8, NT>(y, as_gc4(pb), lane); };
        Blk x0, y0, x1, y1;
        u32 c = c0;
        load(x0, y0, ptr(da, c), ptr(db, c));
        u64 a1 = ptr(da, c + 1u), b1 = ptr(db, c + 1u), a2 = ptr(da, c + 2u), b2 = ptr(db, c + 2u);
        for (; c + 2u < c1; c += 2u) {
            load(x1, y1, a1, b1);
            const u64 a3 = ptr(da, c + 3u), b3 = ptr(db, c + 3u);
            dist_eat(x0, y0, cab, ca, cb);
            load(x0, y0, a2, b2);
            const u64 a4 = ptr(da, c + 4u), b4 = ptr(db, c + 4u);
            dist_eat(x1, y1, cab, ca, cb);
            a1 = a3; b1 = b3; a2 = a4; b2 = b4;
        }
        if (c + 1u < c1) { load(x1, y1, a1, b1); dist_eat(x0, y0, cab, ca, cb); dist_eat(x1, y1, cab, ca, cb); }
        else dist_eat(x0, y0, cab, ca, cb);
        cab = wave_sum(cab); ca = wave_sum(ca); cb = wave_sum(cb);
    }
    count3_fanin_fold(cab, ca, cb, fold, lane, wave);
}

// any block kinds, any lengths (missing blocks are NULL): the persistent walk of k_count_op2_loop -- descriptors one column
// ahead, every load of a column issued before anything is decoded, GAP blocks set into the wave's LDS block from registers.
// `safe`: 16 readable bytes for the unconditional loads of a NULL / FULL operand.
template <bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void k_distance_pair_loop(const u64* __restrict__ da, u32 na, const u64* __restrict__ db, u32 nbk, u32 nblocks,
                          const u64* __restrict__ safe, FoldOut fold)
{
    __shared__ u32 lds[4 * 2048];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    u32* l = lds + wave * 2048u;
    const u32 total = gridDim.x * 4u;
    u32 cab = 0, ca = 0, cb = 0;
    u32 c = uniform32(blockIdx.x * 4u + wave);
    auto raw = [&](const u64* __restrict__ d, u32 n, u32 col) -> u64 { return col < n ? d[col] : 0ull; };
    u64 ar = raw(da, na, c), br = raw(db, nbk, c);
    for (; c < nblocks; c += total) {
        const u64 a = uniform64(ar), b = uniform64(br);
        ar = raw(da, na, c + total); br = raw(db, nbk, c + total);
        if (DESC_K(a) == K_NULL && DESC_K(b) == K_NULL) continue;
        Blk x, y;
        op2_issue<NT>(a, safe, x, lane);
        op2_issue<NT>(b, safe, y, lane);
        __builtin_amdgcn_sched_barrier(0);
        op2_finish(a, x, l, lane);
        op2_finish(b, y, l, lane);
        dist_eat(x, y, cab, ca, cb);
    }
    cab = wave_sum(cab); ca = wave_sum(ca); cb = wave_sum(cb);
    count3_fanin_fold(cab, ca, cb, fold, lane, wave);
}

// ---- all pairs ------------------------------------------------------------------------------------------------------------
#define DM_T  64u              // vectors per tile side
#define DM_K  128u             // words of a block staged per chunk (16 chunks per block)
#define DM_LD (DM_K + 4u)      // LDS row pitch in words: +16 B so that rows r and r+1 start 4 banks apart
#define DM_PIECES (DM_K / 4u)  // 16-byte pieces per staged row chunk
#define DM_STAGE_ITERS (2u * DM_T * DM_PIECES / 256u)   // pieces per thread per chunk (16)
#define DM_LDS_BYTES (2u * DM_T * DM_LD * 4u)           // 67,584 B: two workgroups per CU

// Operand table (device): desc[n] (u64: the vector's descriptor table, 0 = an empty vector), then nblk[n] (u32).
// A-row i is entry i, B-row j is entry b_off + j (b_off = 0 for the symmetric form, where B = A).
struct DmTab { const u64* tab; u32 n; u32 b_off; };

__device__ __forceinline__ u64 dm_desc(DmTab t, u32 e, u32 c)
{
    const u64 dt = t.tab[e];
    const u32 nb = reinterpret_cast<const u32*>(t.tab + t.n)[e];
    return (dt && c < nb) ? reinterpret_cast<const u64*>(dt)[c] : 0ull;
}

// Workgroup = (tile pair, column split).  Thread t owns A-rows ri + 16 r and B-rows ci + 16 c (r, c < 4; ri = t >> 4,
// ci = t & 15): the 16 B-rows a wave reads at one k start 4 banks apart (pitch DM_LD), so a ds_read_b128 touches each bank
// once; the 4 A-rows of a wave are broadcast.  Per 4 staged words: 8 ds_read_b128 and 16 x (4 AND + 4 bcnt) VALU.
// u32 counters: a split spans at most 65,535 columns (host: dm_plan), so a counter never exceeds 65,535 x 65,536 < 2^32.
// out: u64 [na][nb], zeroed by the host; partial tiles add with global_atomic_add_x2.  Symmetric form (sym): tile pairs
// ti <= tj only; an off-diagonal tile adds its transpose as well.
__global__ __launch_bounds__(256, 2)
void k_distance_tile(DmTab t, u32 na, u32 nb, const u32* __restrict__ pairs, u32 cols_per_split, u32 ncols, int sym,
                     const u64* __restrict__ zero16, u64* __restrict__ out)
{
    extern __shared__ u32x4 dm_sm[];                     // [2 * DM_T][DM_LD / 4]: A rows, then B rows
    __shared__ u64 rdesc[2u * DM_T];
    const u32 tid = threadIdx.x, lane = lane_id();
    const u32 pr = pairs[blockIdx.x];
    const u32 ti = pr & 0xFFFFu, tj = pr >> 16;
    const u32 c0 = blockIdx.y * cols_per_split;
    const u32 c1 = c0 + cols_per_split < ncols ? c0 + cols_per_split : ncols;
    const u32 ri = tid >> 4, ci = tid & 15u;
    u32 acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0u;
    (void)lane;

    // the staging pieces of this thread: piece p = i * 256 + tid -> row p / DM_PIECES, 16-B piece p % DM_PIECES
    for (u32 c = c0; c < c1; ++c) {
        u32 kd = K_NULL;
        if (tid < 2u * DM_T) {
            const bool is_a = tid < DM_T;
            const u32 row = is_a ? ti * DM_T + tid : tj * DM_T + (tid - DM_T);
            const bool valid = row < (is_a ? na : nb);
            const u64 d = valid ? dm_desc(t, is_a ? row : t.b_off + row, c) : 0ull;
            rdesc[tid] = d;
            kd = DESC_K(d);
        }
        // (a GAP kind cannot arrive here: the host expanded those blocks)
        const int any_a = __syncthreads_or(tid < DM_T && kd != K_NULL);
        const int any_b = __syncthreads_or(tid >= DM_T && tid < 2u * DM_T && kd != K_NULL);
        if (!any_a || !any_b) continue;                  // workgroup-uniform: nothing of this column can be counted

        u32x4 st[DM_STAGE_ITERS];
        auto fetch = [&](u32 k0) {
#pragma unroll
            for (u32 i = 0; i < DM_STAGE_ITERS; ++i) {
                const u32 p = i * 256u + tid, row = p / DM_PIECES, pc = p % DM_PIECES;
                const u64 d = rdesc[row];
                const u32 k = DESC_K(d);
                // unconditional load (a NULL / FULL row reads the 16 zero bytes), selected afterwards
                gcptr4 src = k == K_BIT ? as_gc4(DESC_P(d)) + (k0 / 4u + pc) : as_gc4(zero16);
                u32x4 v = *src;
                st[i] = k == K_FULL ? (u32x4)(~0u) : v;
            }
        };
        fetch(0u);
        for (u32 k0 = 0; k0 < BMX_BLOCK_WORDS; k0 += DM_K) {
            __syncthreads();                             // the previous chunk has been consumed
#pragma unroll
            for (u32 i = 0; i < DM_STAGE_ITERS; ++i) {
                const u32 p = i * 256u + tid, row = p / DM_PIECES, pc = p % DM_PIECES;
                dm_sm[row * (DM_LD / 4u) + pc] = st[i];
            }
            __syncthreads();
            if (k0 + DM_K < BMX_BLOCK_WORDS) fetch(k0 + DM_K);   // next chunk in flight while this one is counted
            const u32x4* A = dm_sm;
            const u32x4* B = dm_sm + DM_T * (DM_LD / 4u);
#pragma unroll 4
            for (u32 kk = 0; kk < DM_PIECES; ++kk) {
                u32x4 a[4], b[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) a[r] = A[(ri + 16u * r) * (DM_LD / 4u) + kk];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = B[(ci + 16u * q) * (DM_LD / 4u) + kk];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[r][q] += __popc(a[r].x & b[q].x) + __popc(a[r].y & b[q].y) + __popc(a[r].z & b[q].z) + __popc(a[r].w & b[q].w);
            }
        }
        __syncthreads();                                 // rdesc / dm_sm are rewritten by the next column
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u32 i = ti * DM_T + ri + 16u * r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32 j = tj * DM_T + ci + 16u * q;
            if (i < na && j < nb && acc[r][q]) {
                atomicAdd(reinterpret_cast<unsigned long long*>(out + (size_t)i * nb + j), (unsigned long long)acc[r][q]);
                if (sym && ti != tj)
                    atomicAdd(reinterpret_cast<unsigned long long*>(out + (size_t)j * na + i), (unsigned long long)acc[r][q]);
            }
        }
    }
}

// GAP blocks -> bit-blocks for the tile kernel: dout = din with every GAP block replaced by a bit-block in `slab`
// (slots handed out by a bump counter; the host sized the slab by the vector's GAP block count).  A wave per block.
__global__ __launch_bounds__(256)
void k_gap_expand(const u64* __restrict__ din, u32 nblocks, u64* __restrict__ dout, uint4* __restrict__ slab, u32* __restrict__ cursor)
{
    __shared__ u32 lds[4 * 2048];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 nb = uniform32(blockIdx.x * 4u + wave);
    if (nb >= nblocks) return;
    const u64 d = uniform64(din[nb]);
    if (DESC_K(d) != K_GAP) { if (lane == 0) dout[nb] = d; return; }
    u32 slot = 0;
    if (lane == 0) slot = atomicAdd(cursor, 1u);
    slot = __shfl(slot, 0, 64);
    Blk b;
    blk_from_desc(d, b, lds + wave * 2048u, lane);
    uint4* dst = slab + (size_t)slot * 512u;
    blk_store(b, as_g4(dst), lane);
    if (lane == 0) dout[nb] = DESC_MAKE(dst, K_BIT);
}

// |v| of every vector of an operand table (entries e0 .. e0 + n - 1; blocks NULL / FULL / bit only) -> out[0 .. n)
// grid (column workgroups, n): a wave walks every (gridDim.x * 4)-th column of its vector; one atomic per workgroup
__global__ __launch_bounds__(256)
void k_distance_counts(DmTab t, u32 e0, u64* __restrict__ out)
{
    __shared__ u32 part[4];
    const u32 lane = lane_id(), wave = threadIdx.x >> 6;
    const u32 e = e0 + blockIdx.y;
    const u64 dt = t.tab[e];
    const u32 nb = reinterpret_cast<const u32*>(t.tab + t.n)[e];
    u32 cnt = 0;
    if (dt) {
        const u64* desc = reinterpret_cast<const u64*>(dt);
        for (u32 c = blockIdx.x * 4u + wave; c < nb; c += gridDim.x * 4u) {
            const u64 d = uniform64(desc[c]);
            const u32 k = DESC_K(d);
            if (k == K_FULL) cnt += lane == 0 ? 65536u : 0u;
            else if (k == K_BIT) { Blk b; blk_load(b, as_gc4(DESC_P(d)), lane); cnt += blk_lane_popcount(b); }
        }
    }
    cnt = wave_sum(cnt);
    if (lane == 0) part[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 s = (u64)part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + blockIdx.y), (unsigned long long)s);
    }
}

// symmetric form: |a_i| is the diagonal of the AND matrix
__global__ __launch_bounds__(256)
void k_distance_diag(const u64* __restrict__ m, u32 n, u64* __restrict__ ca, u64* __restrict__ cb)
{
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 v = m[(size_t)i * n + i];
    if (ca) ca[i] = v;
    if (cb) cb[i] = v;
}
