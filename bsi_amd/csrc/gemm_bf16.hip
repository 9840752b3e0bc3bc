// bf16 GEMM for gfx950:  C[M,N] = A[M,K] . W[N,K]^T, fp32 accumulation on v_mfma_f32_16x16x32_bf16,
// fused epilogues (bias / GELU / SiLU / gated residual / positional embedding).
//
// Replaces every nn.Linear on the DiT path of the reference (bsi/models/dit.py:33-34,71-81,154,163-165,
// bsi/nn/mlp.py:34-38) together with the elementwise ops torch runs after it.
//
// Design (MI355X-first):
//   * workgroup tile BM x BN x 64 with 64-lane waves arranged WM x WN; every wave owns a
//     (16*TM) x 64 output sub-tile = TM x 4 MFMA tiles, accumulators stay in registers for the whole K loop;
//   * both operands are K-contiguous, so a tile row is 128 B = 8 chunks of 16 B; tiles are staged
//     HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double buffered;
//   * LDS image is lane-linear per wave-instruction (hardware rule); bank conflicts are removed by
//     XOR-ing the chunk index on the *global source* side and again on the ds_read side:
//         activation rows:  chunk' = chunk ^ ((row >> 1) & 7)
//         weight rows:      chunk' = chunk ^ (((row >> 1) & 1) | (((row >> 4) & 3) << 1))
//     both of which reduce to `^ ((lane >> 1) & 7)` for the fragment reads below, making every
//     ds_read_b128 conflict free;
//   * the MFMA is issued as D = Wfrag x Xfrag, i.e. D rows are output columns n and D columns are output
//     rows m.  MFMA row rho of n-tile i is mapped to n = 16*(rho>>2) + 4*i + (rho&3), so after the K loop
//     a lane owns 16 *contiguous* n for each of its rows: the epilogue loads/stores 32-64 B per lane and
//     full 128-B lines per row per wave (no LDS transpose, no scattered 2-byte stores);
//   * workgroup ids are remapped so that each XCD (private L2) walks a contiguous range of tiles with n
//     fastest: the A panel of an m-tile is fetched from HBM once and re-used from that XCD's L2.
#include <cstdlib>

#include "common.h"

namespace {

constexpr int BK = 64;          // K elements per tile
constexpr int ROW_BYTES = 128;  // BK * sizeof(bf16)

struct GemmParams {
    const __bf16* A;
    const __bf16* W;
    const float* bias;
    void* out;
    int M, N, K;
    int lda, ldw, ldo;
    const float* gate;
    int gate_rows, gate_stride;
    int tokens;
    const float* pos;
    const void* aux;  // MUL_GELUGRAD: pre-activation (bf16, layout of out)
    void* out2;       // BIAS_GELU_DUAL: pre-activation output (bf16, layout of out)
    float* colsum;    // MUL_GELUGRAD (K = 64 kernel): [ceil(M / 128)][N] column sums of the output rows of a wave tile, or null
    int tiles_m, tiles_n;
    int gm;       // rasterisation: tiles are walked in bands of gm m-tiles, m fastest inside a band
    // split-K (small M, gemm_bf16_pring_kernel with an fp32 epilogue only): workgroup tile index = split * tiles_m*tiles_n + tile;
    // split s multiplies the K range [s*kslice, (s+1)*kslice) and writes its partial sums to out + s*slab_stride floats
    int splits, kslice;
    size_t slab_stride;
    // grouped launch (gemm_bf16_pring_kernel, fp32 epilogue, exclusive with splits): `groups` problems of one shape whose operands lie at
    // uniform byte strides; workgroup tile index = group * tiles_m*tiles_n + tile
    int groups;
    size_t g_a, g_w, g_bias, g_out;
    unsigned* queue;  // DYN instances of the K = 64 kernel: the stream's tile-queue control block (common.h)
};

// tile index -> (tm, tn): the tiles are walked in bands of gm m-tiles, m fastest inside a band.  An XCD runs 32 consecutive tiles
// together: a gm x (32/gm) block that moves along n and then down the bands.  (An n-stationary order that keeps an XCD's weight
// panels from round to round was measured in round 3: +-1 %, tools/experiments/gemm_variants.inc keeps it.)
__device__ __forceinline__ void tile_coords(const GemmParams& p, int t, int& tm, int& tn) {
    const int band_tiles = p.gm * p.tiles_n;
    const int band = t / band_tiles;
    const int r = t - band * band_tiles;
    const int rows = min(p.gm, p.tiles_m - band * p.gm);  // last band may be short
    tm = band * p.gm + r % rows;
    tn = r / rows;
}

template <int EPI>
struct EpiTraits {
    static constexpr bool out_bf16 = (EPI == BSI_EPI_BIAS_BF16 || EPI == BSI_EPI_BIAS_GELU_BF16 ||
                                      EPI == BSI_EPI_BIAS_SILU_BF16 || EPI == BSI_EPI_BIAS_GELU_DUAL ||
                                      EPI == BSI_EPI_MUL_GELUGRAD_BF16);
};

// XCD-aware bijective remap of the linear workgroup id (guide §5.5 T1).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// `scratch`: this wave's private 16 KB of LDS (or nullptr).  With it, bf16 outputs are transposed through LDS so
// that every global_store_dwordx4 instruction writes 8 complete 128-B lines (8 lanes x 16 B per row).  Without it a
// row's line is written as 16-B pieces by several instructions, and the L2 answers such partial-line writes with a
// fill read of the destination line (measured: fabric reads grew by exactly the output size).
template <int TM, int EPI, bool BIAS_IN_ACC = false>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[4][TM], int mw0, int nw0, int lane,
                                              char* scratch = nullptr) {
    // lane owns rows m = mw0 + 16j + (lane&15), columns nb .. nb+15
    const int nb = nw0 + 16 * (lane >> 4);
    const bool nb_ok = nb < p.N;
    float bias[16];
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
        f32x4 bv = (!BIAS_IN_ACC && p.bias && nb_ok) ? *reinterpret_cast<const f32x4*>(p.bias + nb + e) : f32x4{0.f, 0.f, 0.f, 0.f};
        bias[e] = bv[0]; bias[e + 1] = bv[1]; bias[e + 2] = bv[2]; bias[e + 3] = bv[3];
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int m = mw0 + 16 * j + (lane & 15);
        constexpr bool F32_PLAIN = !EpiTraits<EPI>::out_bf16 && EPI != BSI_EPI_GATE_RESID;  // cross-lane exchange: every lane stays
        if ((m >= p.M || !nb_ok) && !F32_PLAIN && !(EpiTraits<EPI>::out_bf16 && scratch && EPI != BSI_EPI_BIAS_GELU_DUAL &&
                                                   EPI != BSI_EPI_MUL_GELUGRAD_BF16))
            continue;
        float v[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * i + r] = BIAS_IN_ACC ? acc[i][j][r] : acc[i][j][r] + bias[4 * i + r];

        if constexpr (EPI == BSI_EPI_BIAS_GELU_DUAL) {  // generic path: direct stores of the pre-activation
            if (m < p.M && nb_ok) {
                u32x4 a0, a1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                    a1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
                }
                __bf16* o2 = reinterpret_cast<__bf16*>(p.out2) + (size_t)m * p.ldo + nb;
                __builtin_nontemporal_store(a0, reinterpret_cast<u32x4*>(o2));
                __builtin_nontemporal_store(a1, reinterpret_cast<u32x4*>(o2 + 8));
            }
        }
        if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
            if (m < p.M && nb_ok) {
                const __bf16* ax = reinterpret_cast<const __bf16*>(p.aux) + (size_t)m * p.ldo + nb;
                const u32x4 x0 = *reinterpret_cast<const u32x4*>(ax), x1 = *reinterpret_cast<const u32x4*>(ax + 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[2 * e] *= gelu_tanh_grad_f(__uint_as_float(x0[e] << 16));
                    v[2 * e + 1] *= gelu_tanh_grad_f(__uint_as_float(x0[e] & 0xffff0000u));
                    v[8 + 2 * e] *= gelu_tanh_grad_f(__uint_as_float(x1[e] << 16));
                    v[8 + 2 * e + 1] *= gelu_tanh_grad_f(__uint_as_float(x1[e] & 0xffff0000u));
                }
            }
        }
        if constexpr (EPI == BSI_EPI_BIAS_GELU_BF16 || EPI == BSI_EPI_BIAS_GELU_DUAL) {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = gelu_tanh_f(v[e]);
        } else if constexpr (EPI == BSI_EPI_BIAS_SILU_BF16) {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = silu_f(v[e]);
        }

        if constexpr (EpiTraits<EPI>::out_bf16) {
            u32x4 w0, w1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                w1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
            }
            if (scratch && EPI != BSI_EPI_BIAS_GELU_DUAL && EPI != BSI_EPI_MUL_GELUGRAD_BF16) {
                // row r of the wave's [16*TM][128 B] image, 16-B chunks XOR-swizzled by (r & 7)
                const int r = 16 * j + (lane & 15), q2 = (lane >> 4) * 2;
                *reinterpret_cast<u32x4*>(scratch + r * 128 + (((q2) ^ (r & 7)) << 4)) = w0;
                *reinterpret_cast<u32x4*>(scratch + r * 128 + (((q2 + 1) ^ (r & 7)) << 4)) = w1;
            } else {
                __bf16* o = reinterpret_cast<__bf16*>(p.out) + (size_t)m * p.ldo + nb;
                __builtin_nontemporal_store(w0, reinterpret_cast<u32x4*>(o));
                __builtin_nontemporal_store(w1, reinterpret_cast<u32x4*>(o + 8));
            }
        } else {
            float* o = reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + nb;
            if constexpr (EPI == BSI_EPI_GATE_RESID) {
                const int row = (m / p.tokens) % p.gate_rows;
                const float* g = p.gate + (size_t)row * p.gate_stride + nb;
#pragma unroll
                for (int e = 0; e < 16; e += 4) {
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
                    f32x4 xv = *reinterpret_cast<const f32x4*>(o + e);
#pragma unroll
                    for (int r = 0; r < 4; ++r) xv[r] = xv[r] + gv[r] * v[e + r];
                    *reinterpret_cast<f32x4*>(o + e) = xv;
                }
            } else {
                if constexpr (EPI == BSI_EPI_BIAS_POS_F32) {
                    const float* ps = p.pos + (size_t)(m % p.tokens) * p.N + nb;
#pragma unroll
                    for (int e = 0; e < 16 && m < p.M && nb_ok; e += 4) {
                        const f32x4 pv = *reinterpret_cast<const f32x4*>(ps + e);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[e + r] += pv[r];
                    }
                }
                // fp32 rows: 4 x 4 transpose across the four 16-lane groups, so that the 4 lanes of a row write 64 contiguous
                // bytes per store instruction instead of four 16-B pieces 64 B apart (the skip-convolution input gradient of the
                // UNet, M x 256 x 128, ran at 0.7 TB/s of fp32 output with the scattered non-temporal pieces)
                f32x4 r4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) r4[e] = f32x4{v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]};
                transpose_lane_groups(r4);
                if (m < p.M) {
                    const int col = nw0 + 4 * (lane >> 4);
                    float* ot = reinterpret_cast<float*>(p.out) + (size_t)m * p.ldo + col;
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4)
                        if (col + 16 * s4 < p.N) *reinterpret_cast<f32x4*>(ot + 16 * s4) = r4[s4];
                }
            }
        }
    }
    if constexpr (EpiTraits<EPI>::out_bf16 && EPI != BSI_EPI_BIAS_GELU_DUAL && EPI != BSI_EPI_MUL_GELUGRAD_BF16) {
        if (scratch) {
            // the wave reads back its own writes: LDS accesses of one wave are ordered, only the counter must drain
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int rr = lane >> 3, ch = lane & 7;
            const bool cols_ok = nw0 + 8 * ch < p.N;
#pragma unroll
            for (int t = 0; t < 2 * TM; ++t) {
                const int r = 8 * t + rr;
                const u32x4 d = *reinterpret_cast<const u32x4*>(scratch + r * 128 + ((ch ^ (r & 7)) << 4));
                const int m = mw0 + r;
                if (m < p.M && cols_ok)
                    __builtin_nontemporal_store(
                        d, reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(p.out) + (size_t)m * p.ldo + nw0 + 8 * ch));
            }
        }
    }
}

template <int TM, int WM, int WN, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_bf16_kernel(const GemmParams p) {
    constexpr int NW = WM * WN;
    constexpr int NT = NW * 64;
    constexpr int BM = WM * TM * 16;
    constexpr int BN = WN * 64;
    constexpr int ROWS = BM + BN;             // LDS rows per buffer (activation rows first, then weight rows)
    constexpr int BUF_BYTES = ROWS * ROW_BYTES;
    constexpr int STAGE_INSTR = ROWS * 8 / NT;  // global_load_lds per thread per K tile
    static_assert(ROWS * 8 % NT == 0, "tile does not divide over the workgroup");
    static_assert(BM % 8 == 0 && BN % 8 == 0, "8 rows per wave-instruction");

    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    const int nwg = p.tiles_m * p.tiles_n;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- staging addresses: wave-instruction q of this wave fills LDS rows [8*(q*NW+wave), +8) --------
    const int srow = lane >> 3;   // row within the 8-row group
    const int schunk = lane & 7;  // LDS chunk position within the row
    const char* gsrc[STAGE_INSTR];
#pragma unroll
    for (int q = 0; q < STAGE_INSTR; ++q) {
        const int r = (q * NW + wave) * 8 + srow;  // LDS row of this lane
        if (r < BM) {
            const int c = schunk ^ ((r >> 1) & 7);
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;
            gsrc[q] = reinterpret_cast<const char*>(p.A + (size_t)m * p.lda) + c * 16;
        } else {
            const int rw = r - BM;
            const int c = schunk ^ (((rw >> 1) & 1) | (((rw >> 4) & 3) << 1));
            int n = n0 + rw;
            n = n < p.N ? n : p.N - 1;
            gsrc[q] = reinterpret_cast<const char*>(p.W + (size_t)n * p.ldw) + c * 16;
        }
    }

    auto stage = [&](int kt, int buf) {
        char* base = lds + buf * BUF_BYTES;
#pragma unroll
        for (int q = 0; q < STAGE_INSTR; ++q) {
            char* dst = base + (q * NW + wave) * 8 * ROW_BYTES;  // wave-uniform; hardware adds lane*16
            __builtin_amdgcn_global_load_lds(GLB_PTR(gsrc[q] + (size_t)kt * ROW_BYTES), LDS_PTR(dst), 16, 0, 0);
        }
    };

    // ---- fragment read offsets (bytes, relative to the buffer base) --------------------------------
    const int fx = (lane >> 1) & 7;
    // activation fragment of m-tile jm, k-step ks: row wm*TM*16 + 16*jm + (lane&15), chunk (4ks + lane>>4) ^ fx
    const int xoff = (wm * TM * 16 + (lane & 15)) * ROW_BYTES;
    // weight fragment of n-tile i: row BM + wn*64 + 16*((lane&15)>>2) + 4i + (lane&3)
    const int woff = (BM + wn * 64 + 16 * ((lane & 15) >> 2) + (lane & 3)) * ROW_BYTES;
    const int c0 = (((lane >> 4)) ^ fx) << 4;
    const int c1 = (((lane >> 4) + 4) ^ fx) << 4;

    // bf16-output epilogues: the accumulators START at the bias of their column, exactly as in the K = 64 ring kernel that takes
    // these epilogues for M > 128 -- the same fp32 summation order on both sides of that threshold, so a result does not depend on
    // how many rows were computed with it (the conditioning tables of a batch vs. of its halves: bit-identical)
    constexpr bool BIAS_IN_ACC = EpiTraits<EPI>::out_bf16;
    f32x4 acc[4][TM];
    {
        f32x4 bv[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (BIAS_IN_ACC) {
            const int nb = n0 + wn * 64 + 16 * (lane >> 4);
            if (p.bias && nb < p.N) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const f32x4*>(p.bias + nb + 4 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) acc[i][j] = bv[i];
    }

    const int nk = p.K / BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const char* b = lds + buf * BUF_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int cc = ks ? c1 : c0;
            bf16x8 wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                wf[i] = *reinterpret_cast<const bf16x8*>(b + woff + i * 4 * ROW_BYTES + cc);
#pragma unroll
            for (int j = 0; j < TM; ++j) {
                const bf16x8 xf = *reinterpret_cast<const bf16x8*>(b + xoff + j * 16 * ROW_BYTES + cc);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf, acc[i][j], 0, 0, 0);
            }
        }
    }

    gemm_epilogue<TM, EPI, BIAS_IN_ACC>(p, acc, m0 + wm * TM * 16, n0 + wn * 64, lane);
}

// Training epilogues of the K = 64 kernel -- BIAS_GELU_DUAL (two outputs) and MUL_GELUGRAD (an auxiliary input) -- one 16-row block
// at a time with a scheduling fence behind each: interleaved by the compiler, the blocks' temporaries pushed the kernel over its
// 256 registers, it spilled the issue stream's source offsets, and their reloads (scratch loads + s_waitcnt vmcnt(0)) drained the
// operand DMA pipeline in EVERY load phase: 840-860 TFLOP/s against the 1250 of the plain bf16 epilogue at the same shape.  The
// auxiliary rows are fetched two blocks ahead (in front of the stores of the block in between: vmcnt retires in order, and a load
// queued behind stores waits for them), and the pre-activation leaves as whole 128-B lines like the main output.
template <int EPI>
__device__ __forceinline__ void wave_tile_epilogue_train(const GemmParams& p, f32x4 (&acc)[4][8], int mw0, int nw0, int lane) {
    static_assert(EPI == BSI_EPI_BIAS_GELU_DUAL || EPI == BSI_EPI_MUL_GELUGRAD_BF16, "training epilogues only");
    const int rho = lane & 15, qd = lane >> 4;
    const int nb = nw0 + 16 * qd;
    const bool nb_ok = nb < p.N;
    const bool odd = lane & 1;
    const int col = nb + (odd ? 8 : 0);
    // lanes rho and rho^1 swap one half of their 16 columns: 8 lanes then write one complete 128-B line of a row pair per store
    auto store_pair = [&](void* outp, int j, const u32x4 w0, const u32x4 w1) {
        u32x4 st_even, st_odd;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned send = odd ? w0[e] : w1[e];
            const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xf, 0xf, true);  // lane ^ 1
            st_even[e] = odd ? recv : w0[e];
            st_odd[e] = odd ? w1[e] : recv;
        }
        const int m_even = mw0 + 16 * j + (rho & ~1);
        if (nb_ok) {
            __bf16* ob = reinterpret_cast<__bf16*>(outp) + col;
            if (m_even < p.M) __builtin_nontemporal_store(st_even, reinterpret_cast<u32x4*>(ob + (size_t)m_even * p.ldo));
            if (m_even + 1 < p.M) __builtin_nontemporal_store(st_odd, reinterpret_cast<u32x4*>(ob + (size_t)(m_even + 1) * p.ldo));
        }
    };
    // The auxiliary loads are inline asm with hand-counted waits: hipcc assumes loads and stores may complete out of order with each
    // other and would wait vmcnt(0) -- i.e. for the previous blocks' stores -- in front of every block (on this hardware they retire in
    // issue order, MI355X_MICROARCH.md).  Counting needs every store of the wave to be issued: full blocks only, else vmcnt(0).
    const bool full = __builtin_amdgcn_readfirstlane((mw0 + 128 <= p.M && nw0 + 64 <= p.N) ? 1 : 0) != 0;
    u32x4 ax[2][2];
    auto load_aux = [&](int j, u32x4 (&d)[2]) {  // rows / columns beyond the matrix are clamped: their products are never stored
        int m = mw0 + 16 * j + rho;
        m = m < p.M ? m : p.M - 1;
        const __bf16* a = reinterpret_cast<const __bf16*>(p.aux) + (size_t)m * p.ldo + (nb_ok ? nb : 0);
        asm volatile("global_load_dwordx4 %0, %2, off nt\n\tglobal_load_dwordx4 %1, %2, off offset:16 nt"
                     : "=&v"(d[0]), "=&v"(d[1]) : "v"(a) : "memory");
    };
    // ONE wait statement carries the loaded registers ("+v": their uses cannot move in front of it); the drain of partial blocks is
    // a separate operand-free statement.  (With the two waits in the arms of an if / else, each with the operands, hipcc merged
    // the arms' registers by COPYING the loaded registers in front of the wait of one arm -- stale data; tools/check_asm_loads.py
    // now scans the generated code for any read of an inline-asm load's destination before its wait.)
    auto wait_aux = [&](int j, u32x4 (&d)[2]) {  // operations issued after block j's loads: see the sequence in the loop
        if (!full) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (j == 0) asm volatile("s_waitcnt vmcnt(2) ; data of %0 %1" : "+v"(d[0]), "+v"(d[1]) :: "memory");
        else if (j == 1 || j == 7) asm volatile("s_waitcnt vmcnt(4) ; data of %0 %1" : "+v"(d[0]), "+v"(d[1]) :: "memory");
        else asm volatile("s_waitcnt vmcnt(6) ; data of %0 %1" : "+v"(d[0]), "+v"(d[1]) :: "memory");
    };
    // optional column sums of the tile's output rows (GemmParams::colsum): 16 per lane, accumulated over the 8 row blocks
    const bool colsum = EPI == BSI_EPI_MUL_GELUGRAD_BF16 && p.colsum != nullptr;
    float cs[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) cs[e] = 0.f;
    if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
        load_aux(0, ax[0]);
        load_aux(1, ax[1]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * i + r] = acc[i][j][r];  // the accumulators started at the bias
        if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
            // issue order: L0 L1 | block 0: wait L0, compute, L2, S0 | block 1: wait L1, compute, L3, S1 | ... (L / S = 2 instructions)
            wait_aux(j, ax[j & 1]);
            const u32x4 x0 = ax[j & 1][0], x1 = ax[j & 1][1];
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // packed arithmetic: a dword of the auxiliary row = two neighbouring columns
                const f32x2_ g0 = gelu_tanh_grad_f2(f32x2_{__uint_as_float(x0[e] << 16), __uint_as_float(x0[e] & 0xffff0000u)});
                const f32x2_ g1 = gelu_tanh_grad_f2(f32x2_{__uint_as_float(x1[e] << 16), __uint_as_float(x1[e] & 0xffff0000u)});
                const f32x2_ p0 = f32x2_{v[2 * e], v[2 * e + 1]} * g0, p1 = f32x2_{v[8 + 2 * e], v[8 + 2 * e + 1]} * g1;
                v[2 * e] = p0[0]; v[2 * e + 1] = p0[1];
                v[8 + 2 * e] = p1[0]; v[8 + 2 * e + 1] = p1[1];
            }
            if (j + 2 < 8) load_aux(j + 2, ax[j & 1]);
        } else {
            u32x4 a0, a1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                a1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
            }
            store_pair(p.out2, j, a0, a1);
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                const f32x2_ g = gelu_tanh_f2(f32x2_{v[e], v[e + 1]});
                v[e] = g[0];
                v[e + 1] = g[1];
            }
        }
        u32x4 w0, w1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
            w1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
        }
        if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
            if (colsum && mw0 + 16 * j + rho < p.M) {  // the sum of the bf16 values the weight-gradient GEMM will read
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cs[2 * e] += __uint_as_float(w0[e] << 16);
                    cs[2 * e + 1] += __uint_as_float(w0[e] & 0xffff0000u);
                    cs[8 + 2 * e] += __uint_as_float(w1[e] << 16);
                    cs[8 + 2 * e + 1] += __uint_as_float(w1[e] & 0xffff0000u);
                }
            }
        }
        store_pair(p.out, j, w0, w1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
        if (colsum) {  // the 16 lanes of a 16-lane row hold the same columns: DPP row sum, lane rho = 0 stores the wave tile's 16 sums
            f32x4 o4[4];
#pragma unroll
            for (int e = 0; e < 16; ++e) o4[e >> 2][e & 3] = row16_sum(cs[e]);
            if (rho == 0 && nb_ok && mw0 < p.M) {
                float* dst = p.colsum + (size_t)(mw0 >> 7) * p.N + nb;
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(dst + 4 * q) = o4[q];
            }
        }
    }
}

template <int EPI, bool SCRATCH = true, bool BIAS_IN_ACC = false>
__device__ __forceinline__ void wave_tile_epilogue(const GemmParams& p, f32x4 (&acc)[4][8], int mw0, int nw0, int lane, char* scratch) {
    constexpr int TM = 8;
    constexpr bool BF16_OUT = EpiTraits<EPI>::out_bf16;
    const int rho = lane & 15, qd = lane >> 4;

    if constexpr (!SCRATCH && BIAS_IN_ACC && (EPI == BSI_EPI_BIAS_GELU_DUAL || EPI == BSI_EPI_MUL_GELUGRAD_BF16)) {
        wave_tile_epilogue_train<EPI>(p, acc, mw0, nw0, lane);
    } else if constexpr (BF16_OUT) {
        const int nb = nw0 + 16 * qd;
        const bool nb_ok = nb < p.N;
        float bias[16];
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            f32x4 bv = (!BIAS_IN_ACC && p.bias && nb_ok) ? *reinterpret_cast<const f32x4*>(p.bias + nb + e) : f32x4{0.f, 0.f, 0.f, 0.f};
            bias[e] = bv[0]; bias[e + 1] = bv[1]; bias[e + 2] = bv[2]; bias[e + 3] = bv[3];
        }
        const int rr = lane >> 3, ch = lane & 7;
        const bool cols_ok = nw0 + 8 * ch < p.N;
#pragma unroll
        for (int rnd = 0; rnd < TM / 2; ++rnd) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = 2 * rnd + jj;
                float v[16];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[4 * i + r] = BIAS_IN_ACC ? acc[i][j][r] : acc[i][j][r] + bias[4 * i + r];
                if constexpr (EPI == BSI_EPI_MUL_GELUGRAD_BF16) {
                    const int m = mw0 + 16 * j + rho;
                    if (m < p.M && nb_ok) {
                        const __bf16* ax = reinterpret_cast<const __bf16*>(p.aux) + (size_t)m * p.ldo + nb;
                        const u32x4 x0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ax));
                        const u32x4 x1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ax + 8));
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[2 * e] *= gelu_tanh_grad_f(__uint_as_float(x0[e] << 16));
                            v[2 * e + 1] *= gelu_tanh_grad_f(__uint_as_float(x0[e] & 0xffff0000u));
                            v[8 + 2 * e] *= gelu_tanh_grad_f(__uint_as_float(x1[e] << 16));
                            v[8 + 2 * e + 1] *= gelu_tanh_grad_f(__uint_as_float(x1[e] & 0xffff0000u));
                        }
                    }
                }
                if constexpr (EPI == BSI_EPI_BIAS_GELU_DUAL) {  // pre-activation: direct 32-B stores (training only)
                    const int m = mw0 + 16 * j + rho;
                    if (m < p.M && nb_ok) {
                        u32x4 a0, a1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            a0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                            a1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
                        }
                        __bf16* o2 = reinterpret_cast<__bf16*>(p.out2) + (size_t)m * p.ldo + nb;
                        __builtin_nontemporal_store(a0, reinterpret_cast<u32x4*>(o2));
                        __builtin_nontemporal_store(a1, reinterpret_cast<u32x4*>(o2 + 8));
                    }
                }
                if constexpr (EPI == BSI_EPI_BIAS_GELU_BF16 || EPI == BSI_EPI_BIAS_GELU_DUAL) {
#pragma unroll
                    for (int e = 0; e < 16; e += 2) {  // packed: 2.5 instead of 6 vector-ALU instructions per value
                        const f32x2_ g = gelu_tanh_f2(f32x2_{v[e], v[e + 1]});
                        v[e] = g[0];
                        v[e + 1] = g[1];
                    }
                } else if constexpr (EPI == BSI_EPI_BIAS_SILU_BF16) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = silu_f(v[e]);
                }
                u32x4 w0, w1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    w0[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
                    w1[e] = pack_bf16x2(v[8 + 2 * e], v[8 + 2 * e + 1]);
                }
                if constexpr (!SCRATCH) {
                    // lanes rho and rho^1 (rows m, m+1) swap one half of their 16 columns: 8 lanes then write one complete 128-B line
                    const bool odd = lane & 1;
                    u32x4 st_even, st_odd;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned send = odd ? w0[e] : w1[e];
                        const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1, 0xf, 0xf, true);  // lane ^ 1
                        st_even[e] = odd ? recv : w0[e];
                        st_odd[e] = odd ? w1[e] : recv;
                    }
                    const int m_even = mw0 + 16 * j + (rho & ~1);
                    const int col = nb + (odd ? 8 : 0);
                    if (nb_ok) {
                        // non-temporal: the output is consumed by the NEXT kernel; a write-back store allocates in this XCD's L2 and
                        // evicts the A / W panels the other CUs are re-reading
                        __bf16* ob = reinterpret_cast<__bf16*>(p.out) + col;
                        if (m_even < p.M) __builtin_nontemporal_store(st_even, reinterpret_cast<u32x4*>(ob + (size_t)m_even * p.ldo));
                        if (m_even + 1 < p.M) __builtin_nontemporal_store(st_odd, reinterpret_cast<u32x4*>(ob + (size_t)(m_even + 1) * p.ldo));
                    }
                    continue;
                }
                const int r = 16 * jj + rho;  // row within this round's 32-row image
                *reinterpret_cast<u32x4*>(scratch + r * 128 + (((2 * qd) ^ (r & 7)) << 4)) = w0;
                *reinterpret_cast<u32x4*>(scratch + r * 128 + (((2 * qd + 1) ^ (r & 7)) << 4)) = w1;
            }
            if constexpr (!SCRATCH) continue;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            u32x4 d[4];
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int r = 8 * t4 + rr;
                d[t4] = *reinterpret_cast<const u32x4*>(scratch + r * 128 + ((ch ^ (r & 7)) << 4));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
                const int m = mw0 + 32 * rnd + 8 * t4 + rr;
                if (m < p.M && cols_ok)
                    __builtin_nontemporal_store(d[t4], reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(p.out) + (size_t)m * p.ldo + nw0 + 8 * ch));
            }
        }
    } else {
        gemm_epilogue<TM, EPI>(p, acc, mw0, nw0, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // fp32 read-modify-write paths: simple drain
    }
}

// ---------------------------------------------------------------------------------------------------------
// Variant 6: PERSISTENT deep-ring ping-pong (the production schedule).
//   * one workgroup per CU walks its tiles; tile 256 x 256, K step 32, ring of R = 4 slots of 32 KB + 32 KB
//     of per-wave epilogue scratch = the whole 160 KB of LDS;
//   * the DMA stream never stops at a tile boundary: from step nk-D on, the stages issued belong to the NEXT
//     tile, so a tile never starts cold and the previous tile's output stores (16 per wave, issued in E) have
//     2 K steps + the epilogue to retire before a vmcnt wait reaches them (the two L phases after E allow 16
//     extra outstanding operations);
//   * groups A/B alternate L and C phases as in variant 4; the epilogue E of group A runs right after the
//     barrier that ends its last C phase, that of group B right after its last C phase before the barrier,
//     so both epilogues (VALU bound, two waves per SIMD) overlap each other: one epilogue of idle matrix pipe
//     per tile instead of prologue + two epilogues + store drain;
//   * bf16 outputs leave through the LDS scratch in 4 rounds of 32 rows so that every store instruction writes
//     whole 128-B lines.
template <int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_pring_kernel(const GemmParams p) {
    constexpr int TM = 8, NW = 8, R = 4, D = R - 1;
    constexpr int BM = 256, BN = 256;
    constexpr int RB = 64;
    constexpr int SLOT_BYTES = (BM + BN) * RB;
    constexpr int A_BYTES = BM * RB;
    constexpr int KSB = 64;
    constexpr bool BF16_OUT = EpiTraits<EPI>::out_bf16;

    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    char* scratch = lds + R * SLOT_BYTES + wave * 4096;

    const int tiles_mn = p.tiles_m * p.tiles_n;
    const int nwg = p.splits > 1 ? tiles_mn * p.splits : p.groups > 1 ? tiles_mn * p.groups : tiles_mn;
    const int xcd = blockIdx.x & 7, wl = blockIdx.x >> 3;
    const int wpx = (gridDim.x + 7 - xcd) >> 3;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    const int lo = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const int hi = lo + q8 + (xcd < r8 ? 1 : 0);
    int tile = lo + wl;
    if (tile >= hi) return;

    const int srow = lane >> 2, spos = lane & 3;
    const char* gsrc[4];
    auto set_sources = [&](int t) {
        size_t kbytes = 0;  // split-K: byte offset of this split's K range in a row of A / W
        if (p.splits > 1) {
            const int sp = t / tiles_mn;
            t -= sp * tiles_mn;
            kbytes = (size_t)sp * p.kslice * 2;
        }
        const char* Ab = reinterpret_cast<const char*>(p.A);
        const char* Wb = reinterpret_cast<const char*>(p.W);
        if (p.groups > 1) {
            const int gp = t / tiles_mn;
            t -= gp * tiles_mn;
            Ab += (size_t)gp * p.g_a;
            Wb += (size_t)gp * p.g_w;
        }
        int tm_, tn_;
        tile_coords(p, t, tm_, tn_);
        const int m0 = tm_ * BM, n0 = tn_ * BN;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int slot = q * NW + wave;
            if (q < 2) {
                const int r = slot * 16 + srow;
                const int c = spos ^ ((-(r >> 2)) & 3);
                int m = m0 + r;
                m = m < p.M ? m : p.M - 1;
                gsrc[q] = Ab + (size_t)m * p.lda * 2 + c * 16 + kbytes;
            } else {
                const int rw = (slot - 16) * 16 + srow;
                const int c = spos ^ ((-(rw >> 4)) & 3);
                int n = n0 + rw;
                n = n < p.N ? n : p.N - 1;
                gsrc[q] = Wb + (size_t)n * p.ldw * 2 + c * 16 + kbytes;
            }
        }
    };
    auto stage = [&](int kstep, int slot) {
        char* base = lds + slot * SLOT_BYTES;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            char* dst = base + (q * NW + wave) * 1024;
            __builtin_amdgcn_global_load_lds(GLB_PTR(gsrc[q] + (size_t)kstep * KSB), LDS_PTR(dst), 16, 0, 0);
        }
    };

    const int rho = lane & 15, qd = lane >> 4;
    const int cc = ((qd ^ ((-(rho >> 2)) & 3)) << 4);
    const int xoff = (wm * TM * 16 + rho) * RB + cc;
    const int woff = A_BYTES + (wn * 64 + 16 * (rho >> 2) + (rho & 3)) * RB + cc;

    f32x4 acc[4][TM];
    bf16x8 wf[4], xf[TM];
#define PHASE_BARRIER()                          \
    do {                                         \
        __builtin_amdgcn_sched_barrier(0);       \
        __builtin_amdgcn_s_barrier();            \
        __builtin_amdgcn_sched_barrier(0);       \
    } while (0)

    auto epilogue = [&](int t) {
        asm volatile("" : "+s"(t));  // the epilogue's row addresses depend on the tile only: keep them out of the K loop (spills)
        int tm_, tn_;
        if (p.splits > 1) {  // partial sums of split sp go to its slab
            const int sp = t / tiles_mn;
            tile_coords(p, t - sp * tiles_mn, tm_, tn_);
            GemmParams q = p;
            q.out = reinterpret_cast<float*>(p.out) + (size_t)sp * p.slab_stride;
            wave_tile_epilogue<EPI>(q, acc, tm_ * BM + wm * TM * 16, tn_ * BN + wn * 64, lane, scratch);
            return;
        }
        if (p.groups > 1) {  // this group's output and bias
            const int gp = t / tiles_mn;
            tile_coords(p, t - gp * tiles_mn, tm_, tn_);
            GemmParams q = p;
            q.out = reinterpret_cast<char*>(p.out) + (size_t)gp * p.g_out;
            if (p.bias) q.bias = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.bias) + (size_t)gp * p.g_bias);
            wave_tile_epilogue<EPI>(q, acc, tm_ * BM + wm * TM * 16, tn_ * BN + wn * 64, lane, scratch);
            return;
        }
        tile_coords(p, t, tm_, tn_);
        wave_tile_epilogue<EPI>(p, acc, tm_ * BM + wm * TM * 16, tn_ * BN + wn * 64, lane, scratch);
    };

    const int nk = (p.splits > 1 ? p.kslice : p.K) / 32;  // launcher guarantees nk >= D
    set_sources(tile);
#pragma unroll
    for (int d = 0; d < D; ++d) stage(d, d);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (D - 1)) : "memory");
    PHASE_BARRIER();
    if (wm == 1) PHASE_BARRIER();  // group B runs one phase behind

    int slot = 0, pslot = D;
    int after_e = 0;  // L phases since the last epilogue whose stores may still be in flight
    while (true) {
        const int next = tile + wpx;
        const bool has_next = next < hi;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int v = 0; v < nk; ++v) {
            // ---- L(v)
            {
                const char* b = lds + slot * SLOT_BYTES;
#pragma unroll
                for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(b + woff + i * 4 * RB);
#pragma unroll
                for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(b + xoff + j * 16 * RB);
            }
            bool issued = false;
            if (v + D < nk) {
                stage(v + D, pslot);
                issued = true;
            } else if (has_next) {
                if (v + D == nk) set_sources(next);
                stage(v + D - nk, pslot);
                issued = true;
            }
            // the stage of step v+1 must have landed; younger stages (and, right after an epilogue, its 16
            // stores) may stay in flight
            if (issued) {
                if (BF16_OUT && EPI != BSI_EPI_BIAS_GELU_DUAL && after_e > 0)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (D - 1) + 16) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (D - 1)) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (after_e > 0) --after_e;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            PHASE_BARRIER();
            // ---- C(v)
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < TM; ++j)
#pragma unroll
                for (int i0 = 0; i0 < 4; ++i0) {  // boustrophedon, as in the k64r kernel below
                    const int i = (j & 1) ? 3 - i0 : i0;
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
            if (v == nk - 1 && wm == 1) epilogue(tile);  // group B: before the barrier that ends its last C phase
            PHASE_BARRIER();
            slot = (slot == R - 1) ? 0 : slot + 1;
            pslot = (pslot == R - 1) ? 0 : pslot + 1;
        }
        if (wm == 0) epilogue(tile);  // group A: after that barrier, merged with its next L phase
        {   // the store allowance of the next phases is valid only if every store of the epilogue was issued (no M / N tail)
            int tm_, tn_;
            tile_coords(p, (p.splits > 1 || p.groups > 1) ? tile % tiles_mn : tile, tm_, tn_);
            after_e = (tm_ * 256 + 256 <= p.M && tn_ * 256 + 256 <= p.N) ? 2 : 0;
        }
        if (!has_next) break;
        tile = next;
    }
    if (wm == 0) PHASE_BARRIER();
#undef PHASE_BARRIER
}

extern int g_gm;

// ---------------------------------------------------------------------------------------------------------
// Variant 12: 128-B tile rows (whole cache lines per DMA row, see variant 10) on a RING OF FIVE HALF-STAGES.
// A half-stage is the A half (256 rows) or the W half (256 rows) of a K = 64 stage: 32 KB; five slots = all 160 KB of LDS
// (the epilogue needs no scratch: wave_tile_epilogue<.., false>).  One half-stage (4 DMA instructions per wave) is issued
// per load phase, exactly the DMA instruction count of variant 6 but with twice the bytes per LDS-DMA cycle.  With H(A of
// global stage G) = 2G, H(W of G) = 2G+1 and slot = H % 5, load phase P = 2G + ks issues H = P + 3: W(G+1) at ks = 0,
// A(G+2) at ks = 1; everything needed at P+1 has then been in flight for at least two phases (the cover that a 3-slot
// K = 32 ring has and that costs nothing).  The issue stream runs ahead of the compute across tile boundaries with its
// own tile pointer.
// DYN: the tiles are not a static share but TICKETS (common.h, "tile queue"): XCD x's tiles [lo_x, hi_x) are handed out in order by
// the counter queue[x]; a workgroup whose own XCD has run dry draws from the next XCD's counter.  The ticket of the NEXT tile is
// drawn while the current tile computes, by wave 0, in three steps a K stage apart so that nothing ever waits: a returning atomic
// issued in front of a load phase's DMA group (the in-order vmcnt of the following phases covers it), one stage later its value
// stored to the workgroup's mailbox line in global memory (all 160 KB of LDS are ring), one stage later every wave loads the
// mailbox, one stage later the value is in a scalar register -- long before the issue stream, which runs 1.5 stages ahead of the
// arithmetic, crosses into the next tile (K >= 512).  Same tiles, same K order: bit-identical results.
template <int EPI, bool DYN>
__global__ __launch_bounds__(512) void gemm_bf16_k64r_kernel(const GemmParams p) {
    constexpr int TM = 8, NW = 8;
    constexpr int BM = 256, BN = 256, RB = 128;
    constexpr int HALF = 256 * RB;  // 32 KB
    constexpr bool BF16_OUT = EpiTraits<EPI>::out_bf16;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;

    const int nwg = p.tiles_m * p.tiles_n;
    const int xcd = blockIdx.x & 7, wl = blockIdx.x >> 3;
    const int wpx = (gridDim.x + 7 - xcd) >> 3;
    const int q8 = nwg >> 3, r8 = nwg & 7;
    auto xcd_lo = [&](int x) { return (x < r8) ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8; };
    int lo = xcd_lo(xcd);
    int hi = lo + q8 + (xcd < r8 ? 1 : 0);
    const int nk = p.K / 64;
    int tile;
    // DYN state (wave-uniform, identical in all 8 waves: every wave sees the same mailbox values)
    int qx = xcd;             // the XCD whose counter the next ticket is drawn from
    int tries = 8;            // counters not yet found empty
    int ntile = 0;            // the tile after the current one, once `found`
    int extra = -1;           // the tile after THAT, when a ticket stood for two tiles (see the first draw)
    bool found = false;
    int ev = -1, ek = 0;      // ticket pipeline: the K stage of its next step, and the step (0 draw, 1 store, 2 fetch, 3 decode)
    unsigned* const mbox = DYN ? p.queue + BSI_TQ_MBOX + 16 * blockIdx.x : nullptr;
    // The ticket / mailbox value in flight lives in the FIXED register v255, named in the asm text and listed as a clobber: hipcc
    // then counts it as used but, allocating from v0 upwards and needing fewer than 255 registers here, never names it itself --
    // tools/check_asm_loads.py (tests/test_asm_waits.py) verifies that for every build.  A compiler-allocated destination was
    // copied, split or lent to another value while the load was in flight in every earlier form of this code ("+v" operands do not
    // pin a value to ONE register across blocks); accumulator registers are no way out either: an asm statement that names one makes
    // hipcc halve the kernel's VGPR budget (128 + 128: 400-580 bytes of scratch per lane).
    // lane 0 of this wave only: returning atomic +1 on (base + off) -> v255
#define TQ_DRAW(off, base)                                                                                                      \
    do {                                                                                                                        \
        unsigned long long sv_;                                                                                                 \
        asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add v255, %1, %2, %3 sc0\n\ts_mov_b64 exec, %0"   \
                     : "=&s"(sv_) : "v"(off), "v"(1u), "s"(base) : "memory", "v255");                                           \
    } while (0)
    // waits until at most four younger vector-memory operations (a DMA group) are in flight, then reads v255 (lane 0's value, as a scalar)
#define TQ_VALUE(dst)                                                                                                           \
    do {                                                                                                                        \
        unsigned v_;                                                                                                            \
        asm volatile("s_waitcnt vmcnt(4)\n\tv_mov_b32 %0, v255" : "=v"(v_) :: "memory", "v255");                                \
        dst = (unsigned)__builtin_amdgcn_readfirstlane((int)v_);                                                                \
    } while (0)
#ifdef BSI_LAB
    unsigned long long lab_t0 = __builtin_amdgcn_s_memrealtime(), lab_t1 = 0;
    unsigned lab_tiles = 0;
#endif
    if constexpr (DYN) {
        // Ticket T of XCD x's counter stands for TWO tiles while T < W (W = the XCD's workgroups in this grid): tiles T and T + W of
        // the XCD's range -- the first two rounds are dealt as the static schedule deals them (32 neighbouring tiles of an XCD in flight
        // together: drawing two tickets per workgroup instead put every other tile of a 64-tile window in flight, twice the operand
        // panels per round in the XCD's L2: +6 us on the first tile) -- and for ONE tile, T + W, from then on.  The first ticket is
        // drawn by thread 0 before anything is in flight; the ring is still empty, so the values travel through the last words of LDS
        // (slot 4, first written by the fifth half-stage, two barriers from here).  A workgroup that finds its XCD dry -- it started
        // late -- asks the other XCDs in turn.
        unsigned* word = reinterpret_cast<unsigned*>(lds + 5 * HALF - 4);
        if (tid == 0) {
            unsigned t0 = 0xffffffffu, t1 = 0xffffffffu;
            int x = xcd, left = 8;
            while (left > 0) {
                const int n = q8 + (x < r8 ? 1 : 0), w = (int)((gridDim.x + 7 - x) >> 3);
                const unsigned got = n > 0 ? __hip_atomic_fetch_add(p.queue + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
                if (got < (unsigned)w) {
                    if (got < (unsigned)n) t0 = (unsigned)xcd_lo(x) + got;
                    if (got + (unsigned)w < (unsigned)n) t1 = (unsigned)xcd_lo(x) + got + (unsigned)w;
                } else if (got != 0xffffffffu && got + (unsigned)w < (unsigned)n) {
                    t0 = (unsigned)xcd_lo(x) + got + (unsigned)w;
                }
                if (got == 0xffffffffu || got + 2u * (unsigned)w >= (unsigned)n) {  // this counter is dry now or will be at the next draw
                    x = (x + 1) & 7;
                    --left;
                }
                if (t0 != 0xffffffffu) break;
            }
            word[0] = t0;
            word[-1] = t1;
            word[-2] = (unsigned)(x | (left << 8));
        }
        __syncthreads();
        const unsigned t0 = word[0], t1 = word[-1], st = word[-2];
        __syncthreads();
        qx = __builtin_amdgcn_readfirstlane((int)(st & 0xff));
        tries = __builtin_amdgcn_readfirstlane((int)(st >> 8));
        tile = __builtin_amdgcn_readfirstlane((int)t0);
        ntile = __builtin_amdgcn_readfirstlane((int)t1);
        lo = 0;
        hi = nwg;  // `tile < hi` below means "a tile"; no tile = hi
        // every counter dry (a late workgroup): no tile -- it walks through the empty prologue to the end of the kernel, where it is
        // counted as gone.  (No early return: a second copy of the leaving code made hipcc merge the two and fail to select.)
        if (tile < 0) tile = hi;
        found = ntile >= 0;
#ifdef BSI_LAB
        lab_t1 = __builtin_amdgcn_s_memrealtime();
        if (p.splits > 1000) {  // laboratory: align the start of all workgroups to (entry + splits - 1000 ticks of 10 ns)
            while (__builtin_amdgcn_s_memrealtime() - lab_t0 < (unsigned long long)(p.splits - 1000)) __builtin_amdgcn_s_sleep(1);
        }
#endif
    } else {
        tile = lo + wl;
        if (tile >= hi) return;
    }

    // ---- issue stream: half-stages in the order A(0) W(0) A(1) W(1) ... over this workgroup's tiles
    const int srow = lane >> 3, spos = lane & 7;
    unsigned gA[4], gW[4];  // source byte offsets of this lane's chunk for the 4 instructions of a half-stage
    const char* Ab = reinterpret_cast<const char*>(p.A);
    const char* Wb = reinterpret_cast<const char*>(p.W);
    int itile = tile, iv = 0, ihalf = 0, islot = 0;  // next half-stage to issue and its slot
    auto set_sources = [&](int t) {
        int tm_, tn_;
        tile_coords(p, t, tm_, tn_);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (q * NW + wave) * 8 + srow;
            int m = tm_ * BM + r;
            m = m < p.M ? m : p.M - 1;
            int n = tn_ * BN + r;
            n = n < p.N ? n : p.N - 1;
            gA[q] = (unsigned)m * (unsigned)(p.lda * 2) + ((spos ^ ((r >> 1) & 7)) << 4);
            gW[q] = (unsigned)n * (unsigned)(p.ldw * 2) + ((spos ^ (((r >> 1) & 1) | (((r >> 4) & 3) << 1))) << 4);
        }
    };
    auto issue_next = [&]() -> bool {  // issues one half-stage; false when the stream is exhausted
        if (itile >= hi) return false;
        char* base = lds + islot * HALF + wave * 1024;
        const size_t koff = (size_t)iv * 128;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const char* src = ihalf ? Wb + koff + gW[q] : Ab + koff + gA[q];
            __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(base + q * NW * 1024), 16, 0, 0);
        }
        islot = islot == 4 ? 0 : islot + 1;
        if (ihalf) {
            ihalf = 0;
            if (++iv == nk) {
                iv = 0;
                itile = DYN ? (found ? ntile : hi) : itile + wpx;  // DYN: decided by stage nk - 2 (see the K loop)
                if (itile < hi) set_sources(itile);
            }
        } else {
            ihalf = 1;
        }
        return true;
    };

    const int rho = lane & 15, qd = lane >> 4;
    const int xkey = (rho >> 1) & 7, wkey = ((rho >> 1) & 1) | ((rho >> 2) << 1);
    const int xrow = (wm * TM * 16 + rho) * RB;
    const int wrow = (wn * 64 + 16 * (rho >> 2) + (rho & 3)) * RB;

    f32x4 acc[4][TM];
    bf16x8 wf[4], xf[TM];
#define PHASE_BARRIER()                          \
    do {                                         \
        __builtin_amdgcn_sched_barrier(0);       \
        __builtin_amdgcn_s_barrier();            \
        __builtin_amdgcn_sched_barrier(0);       \
    } while (0)

    auto epilogue = [&](int t) {
        // the epilogue's row addresses (16-24 per lane) depend on the tile only; without the fence they are computed in front of the K
        // loop (group B's epilogue sits inside it) and hold up to 48 registers through it -- the training instances spilled
        asm volatile("" : "+s"(t));
        int tm_, tn_;
        tile_coords(p, t, tm_, tn_);
        wave_tile_epilogue<EPI, false, BF16_OUT>(p, acc, tm_ * BM + wm * TM * 16, tn_ * BN + wn * 64, lane, nullptr);
    };
    auto init_acc = [&](int t) {  // bf16 epilogues: accumulators start at the bias of their column (lane owns n = nb .. nb+15)
        f32x4 bv[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (BF16_OUT) {
            int tm_, tn_;
            tile_coords(p, t, tm_, tn_);
            // (Scalar-cache loads of the bias -- four s_load_dwordx16, no vmcnt(0) drain of the previous tile's stores in front of the
            // first accumulator write -- were measured: -0.7 %.  The stall only moves three phases down, to the first operand wait
            // the in-order vmcnt cannot satisfy before the stores have left.)
            const int nb = tn_ * BN + wn * 64 + 16 * qd;
            if (p.bias && nb < p.N) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const f32x4*>(p.bias + nb + 4 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) acc[i][j] = bv[i];
    };

    // prologue: A(0), W(0), A(1) in flight; stage 0 must have landed before the first load phase
    if (tile < hi) set_sources(tile);
    issue_next();
    issue_next();
    bool more = issue_next();
    if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PHASE_BARRIER();
    if (wm == 1) PHASE_BARRIER();  // group B runs one phase behind

    int sa = 0, sw = 1;  // slots of the A and W halves of the stage being consumed
    // Epilogue stores and the in-order vmcnt: a DMA half-stage issued AFTER the stores cannot be waited for without draining
    // them (measured: with the stores first, they had one phase to complete and cost 16 % of the kernel).  So the half-stage
    // of the load phase that follows an epilogue is issued IN FRONT of the epilogue's stores (its slot is free: group A is
    // already in that load phase, group B half a step before it), and the NST stores may stay in flight for the next three
    // phases (allowances 8+NST, 4+NST, 8+NST).
    constexpr int NST = EPI == BSI_EPI_BIAS_GELU_DUAL ? 32 : 16;
    int after_e = 0;          // 3, 2, 1: phases after an epilogue whose stores may still be in flight
    bool pre = false, pre_status = false;  // the next load phase's half-stage was issued in front of the epilogue
    while (tile < hi) {
        init_acc(tile);
        for (int v = 0; v < nk; ++v) {
            const char* ba = lds + sa * HALF;
            const char* bw = lds + sw * HALF;
            if constexpr (DYN) {
                // ---- the ticket pipeline: one step at the TOP of a K stage (in front of its first DMA group), a stage apart; the phases
                // below are the static schedule's, untouched.  The ticket of the tile after this one was drawn by wave 0 at the tile
                // boundary, in front of the epilogue's stores (a returning atomic takes ~1.5 us; the stores' allowance of the next three
                // phases covers it) -> stage 2: wave 0 stores it to the workgroup's mailbox -> stage 3 (the store completed a stage
                // ago, every wave has passed a barrier since): lane 0 of every wave loads the mailbox -> stage 4: all waves decode the
                // same ticket -- long before the issue stream leaves this tile at stage nk - 2.  A counter that is dry, or will be at the
                // next draw (ticket + 2 W >= its tiles), sends the NEXT boundary's draw to the next XCD's counter; a draw that fails
                // ends the workgroup after its current tile (a draw from inside a tile would be waited for half a stage later: ~1 us).
                // The value in flight sits in the reserved register v255 (see TQ_DRAW above).
                if (v == ev) {
                    if (ek == 1) {
                        if (wave == 0) {  // at most the previous phase's DMA group is younger than the atomic: landed
                            unsigned tk;
                            TQ_VALUE(tk);
                            unsigned long long sv_;
                            asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tglobal_store_dword %1, %2, %3 sc1\n\ts_mov_b64 exec, %0"
                                         : "=&s"(sv_) : "v"(0), "v"(tk), "s"(mbox) : "memory");
                        }
                    } else if (ek == 2) {
                        unsigned long long sv_;
                        asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tglobal_load_dword v255, %1, %2 sc1\n\ts_mov_b64 exec, %0"
                                     : "=&s"(sv_) : "v"(0), "s"(mbox) : "memory", "v255");
                    } else {
                        unsigned got;
                        TQ_VALUE(got);
                        const int n = q8 + (qx < r8 ? 1 : 0), w = (int)((gridDim.x + 7 - qx) >> 3);
#ifdef BSI_LAB
                        if (p.gate_rows & 8) {
                            ntile = tile + wpx;
                            found = ntile < xcd_lo(xcd) + q8 + (xcd < r8 ? 1 : 0);
                        } else
#endif
                        if (got < (unsigned)w && got < (unsigned)n) {  // an early ticket of that counter (its own workgroups are late): two tiles
                            ntile = xcd_lo(qx) + (int)got;
                            found = true;
                            if (got + (unsigned)w < (unsigned)n) extra = ntile + w;
                        } else if (got + (unsigned)w < (unsigned)n) {
                            ntile = xcd_lo(qx) + (int)got + w;
                            found = true;
                        }
                        if (got + 2u * (unsigned)w >= (unsigned)n && !(BSI_ABL(p.gate_rows, 8))) {  // dry now, or at the next draw: ask the next XCD then
                            qx = (qx + 1) & 7;
                            --tries;
                        }
                    }
                    if (ek < 3) { ++ek; ev = v + 1; }
                    else ev = -1;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                // ---- L(v, ks): DMA issue (unless it went out in front of an epilogue), fragment reads
                bool issued;
                if (pre) { issued = pre_status; pre = false; }
                else issued = issue_next();
                {
                    const int cx = ((ks * 4 + qd) ^ xkey) << 4, cw = ((ks * 4 + qd) ^ wkey) << 4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(bw + wrow + i * 4 * RB + cw);
#pragma unroll
                    for (int j = 0; j < TM; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(ba + xrow + j * 16 * RB + cx);
                }
                // ks = 0 issued W(G+1): A(G+1) (issued one phase ago) may also stay in flight -> 8; ks = 1 issued A(G+2): the
                // whole stage G+1 must have landed -> 4 (only the new one in flight); + the stores of a recent epilogue.
                if (issued) {
                    if (BF16_OUT && after_e > 0) {
                        if (EPI == BSI_EPI_MUL_GELUGRAD_BF16 && p.colsum != nullptr) {  // + the wave tile's 4 column-sum stores (operand-free waits)
                            if (ks == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 + NST + 4) : "memory");
                            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NST + 4) : "memory");
                        } else if (ks == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 + NST) : "memory");
                        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NST) : "memory");
                    } else if (ks == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (after_e > 0) --after_e;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                PHASE_BARRIER();
                // ---- C(v, ks)
                __builtin_amdgcn_s_setprio(1);
                // boustrophedon over the 4 x TM fragment grid: one operand changes per MFMA instead of two at every row end.  The
                // chip is power limited under this stream and operand toggling is part of the bill: +2 % on a
                // register-only MFMA stream (tools/experiments/mfma_power.hip), +0.5..2.5 % here (profiles/r3/mfma_power.txt)
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int i0 = 0; i0 < 4; ++i0) {
                        const int i = (j & 1) ? 3 - i0 : i0;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
                    }
                __builtin_amdgcn_s_setprio(0);
                if (ks == 1 && v == nk - 1 && wm == 1) {  // group B: before the barrier that ends its last C phase
                    pre_status = issue_next();
                    pre = true;
                    epilogue(tile);
                }
                PHASE_BARRIER();
            }
            sa = sa >= 3 ? sa - 3 : sa + 2;
            sw = sw >= 3 ? sw - 3 : sw + 2;
        }
        // DYN: the ticket of the tile after the NEXT one is drawn here, at the boundary, if there is a next tile and counters remain
        const bool want = DYN && found && extra < 0 && tries > 0 && nk >= 8;
        if (wm == 0) {  // group A: after that barrier, i.e. at the start of its next load phase
            pre_status = issue_next();
            pre = true;
            if constexpr (DYN) {
#ifdef BSI_LAB
                if (p.gate_rows & 8) {}  // laboratory: no atomic (the decode below then walks the static order: timing only)
                else
#endif
                if (want && wave == 0) TQ_DRAW(qx * 4, p.queue);  // in front of the epilogue's stores: their allowance covers it
            }
            epilogue(tile);
        }
        {   // the store allowance of the next phases is valid only if every store of the epilogue is issued (no M / N tail)
            int tm_, tn_;
            tile_coords(p, tile, tm_, tn_);
            after_e = (tm_ * 256 + 256 <= p.M && tn_ * 256 + 256 <= p.N) ? 3 : 0;
        }
#ifdef BSI_LAB
        if (tid == 0 && p.queue && lab_tiles < 8 && blockIdx.x < 256) {  // end of tile `lab_tiles`: (low word of the time, tile index)
            unsigned* e = p.queue + BSI_TQ_MBOX + 16 * (256 + blockIdx.x) + 2 * lab_tiles;
            e[0] = (unsigned)__builtin_amdgcn_s_memrealtime();
            e[1] = (unsigned)tile;
        }
        ++lab_tiles;
#endif
        const int next = DYN ? (found ? ntile : hi) : tile + wpx;
        if (next >= hi) break;
        tile = next;
        if constexpr (DYN) {  // the tile after `next`: the second tile of a two-tile ticket, or the ticket just drawn (stored at stage 2)
            found = extra >= 0;
            ntile = extra;
            extra = -1;
            ev = want ? 2 : -1;
            ek = 1;
        }
    }
    if (wm == 0) PHASE_BARRIER();
#undef PHASE_BARRIER
#undef TQ_DRAW
#undef TQ_VALUE
#ifdef BSI_LAB
    if (tid == 0 && p.queue) {  // laboratory build: per-workgroup stamps in the mailbox line (100 MHz ticks): entry, first ticket known, leaving
        unsigned* mb_ = p.queue + BSI_TQ_MBOX + 16 * blockIdx.x;
        unsigned long long* st = reinterpret_cast<unsigned long long*>(mb_ + 2);
        const unsigned long long prev_leave = st[2];
        st[0] = lab_t0; st[1] = lab_t1; st[2] = __builtin_amdgcn_s_memrealtime();
        reinterpret_cast<unsigned long long*>(mb_ + 10)[0] = prev_leave;
        mb_[1] = lab_tiles;
    }
#endif
    if constexpr (DYN) {  // the last workgroup to leave zeroes the counters for the next launch on this stream
        if (tid == 0) {
            const unsigned gone = __hip_atomic_fetch_add(p.queue + BSI_TQ_GONE + xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gone == (unsigned)wpx - 1) {  // last of this XCD's workgroups
                const unsigned xg = __hip_atomic_fetch_add(p.queue + BSI_TQ_XCDS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned nx = gridDim.x < 8 ? gridDim.x : 8;
                if (xg == nx - 1) {
#pragma unroll
                    for (int i = 0; i <= BSI_TQ_XCDS; ++i) __hip_atomic_store(p.queue + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

template <int TM, int WM, int WN, int EPI>
int launch_cfg(const GemmParams& p0, hipStream_t s) {
    constexpr int BM = WM * TM * 16, BN = WN * 64;
    GemmParams p = p0;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    const size_t lds = 2 * (size_t)(BM + BN) * ROW_BYTES;
    auto kern = gemm_bf16_kernel<TM, WM, WN, EPI>;
    set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(WM * WN * 64), lds, s, p);
    BSI_CHECK_LAUNCH("bsi_gemm_bf16");
    return BSI_OK;
}

int g_variant = 12;  // 12: production (K = 64 half-stage ring + K = 32 ring), 6: K = 32 ring only
int g_gm = 4;  // band height: 4 m-tiles x 8 n-tiles per XCD round minimises L2 misses (PMC: fc1 605 -> 403 MB per launch)
// grids: compute_cus() (common.h) = the CUs of the current device minus those reserved for a concurrent communication kernel

template <int EPI>
int launch_k64r(const GemmParams& p0, hipStream_t s) {
    GemmParams p = p0;
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.gm = g_gm < p.tiles_m ? g_gm : p.tiles_m;
    if (p.gm < 1) p.gm = 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const size_t lds = 5 * (size_t)256 * 128;
    // tile queue (bsi_set_tile_queue): worth it when workgroups take more than one tile, possible when the ticket pipeline fits
    // into a tile (K >= 512); the grid then spans ALL CUs -- the queue, not a reserve, absorbs CUs that are busy elsewhere
    // (on a CU-masked stream the masked-out CUs are not "busy elsewhere" but unreachable: the grid is the partition's size)
    const int avail = g_bsi_cu_masked ? compute_cus() : device_cus();
    const int all = avail < BSI_TQ_MAX_WG ? avail : BSI_TQ_MAX_WG;
    p.queue = (nwg > all && p.K >= 512) ? bsi_tile_queue_block(s) : nullptr;
#ifdef BSI_LAB
    unsigned*& lab_block = g_lab_static_block;  // laboratory build: the static schedule stamps into a block of its own
    if (!p.queue && getenv("BSI_LAB_STAMPS")) {
        if (!lab_block && hipMalloc(reinterpret_cast<void**>(&lab_block), BSI_TQ_WORDS * 4) == hipSuccess) (void)hipMemset(lab_block, 0, BSI_TQ_WORDS * 4);
        GemmParams ps = p;
        ps.queue = lab_block;
        const int grid = nwg < compute_cus() ? nwg : compute_cus();
        auto kern = gemm_bf16_k64r_kernel<EPI, false>;
        set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, ps);
        BSI_CHECK_LAUNCH("bsi_gemm_bf16");
        return BSI_OK;
    }
#endif
    if (p.queue) {
#ifdef BSI_LAB
        if (getenv("BSI_LAB_ALIGN")) p.splits = 1000 + atoi(getenv("BSI_LAB_ALIGN"));
        if (getenv("BSI_LAB_TQ")) p.gate_rows = atoi(getenv("BSI_LAB_TQ"));  // laboratory: mailbox scope variants (see the K loop)
#endif
        auto kern = gemm_bf16_k64r_kernel<EPI, true>;
        set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
        hipLaunchKernelGGL(kern, dim3(all), dim3(512), lds, s, p);
    } else {
        // With the queue on, launches that keep the static schedule also span ALL CUs: with at most one tile per workgroup a
        // reserve only turns one round into two for good, while a late workgroup (its CU held by a communication kernel) costs that
        // second round only while the communication kernel is actually there.  (Short K, or no control block: the reserve applies.)
        const int cus = (g_bsi_tile_queue && nwg <= all) ? all : compute_cus();
        const int grid = nwg < cus ? nwg : cus;
        auto kern = gemm_bf16_k64r_kernel<EPI, false>;
        set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, p);
    }
    BSI_CHECK_LAUNCH("bsi_gemm_bf16");
    return BSI_OK;
}

template <int EPI>
int launch_pring(const GemmParams& p0, hipStream_t s) {
    GemmParams p = p0;
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.gm = g_gm < p.tiles_m ? g_gm : p.tiles_m;
    if (p.gm < 1) p.gm = 1;
    const int nwg = p.tiles_m * p.tiles_n;
    const int grid = nwg < compute_cus() ? nwg : compute_cus();
    const size_t lds = 4 * (size_t)512 * 64 + 32768;
    auto kern = gemm_bf16_pring_kernel<EPI>;
    set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, p);
    BSI_CHECK_LAUNCH("bsi_gemm_bf16");
    return BSI_OK;
}

template <int EPI>
int launch_epi(const GemmParams& p, hipStream_t s) {
    // variant 12 (production): bf16-output epilogues with K >= 128 on the K = 64 half-stage ring, everything else large on the
    // K = 32 ring; variant 6: the K = 32 ring for every epilogue (the A/B partner of the full-size tests)
    if (g_variant == 12 && EpiTraits<EPI>::out_bf16 && p.M > 128 && p.K >= 128 && p.K % 64 == 0) return launch_k64r<EPI>(p, s);
    if (p.M > 128 && p.K >= 96) return launch_pring<EPI>(p, s);
    // Large problems with a short K: 256x256 tile, 8 waves (2x4), wave tile 128x64.
    // Small M (adaLN tables, tiny test models): 64x256 tile, 4 waves (1x4), wave tile 64x64... keeps N coverage.
    if (p.M > 128) return launch_cfg<8, 2, 4, EPI>(p, s);
    return launch_cfg<4, 2, 4, EPI>(p, s);
}

// ---------------------------------------------------------------------------------------------------------
// Split-K for small M (a few images per call: 16..64 tiles on 256 CUs, each walking its whole K loop alone -- 28..75 us per GEMM
// of pure latency).  The K range is cut into `splits` slices; tile (split, m, n) runs the K = 32 ring kernel with the fp32
// epilogue into slab `split` of the caller's workspace, and splitk_finish_kernel sums the slabs in fixed order (deterministic),
// adds the bias, applies the activation and rounds to bf16.
template <int EPI>
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* __restrict__ slabs, size_t slab_stride, int splits,
                                                            const float* __restrict__ bias, int M, int N, int ldo,
                                                            __bf16* __restrict__ out) {
    const int n4 = N >> 2;
    const size_t total = (size_t)M * n4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / n4), c = (int)(i % n4) * 4;
        f32x4 a = bias ? *reinterpret_cast<const f32x4*>(bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < splits; ++sp) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(slabs + (size_t)sp * slab_stride + (size_t)m * N + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += v[e];
        }
        if constexpr (EPI == BSI_EPI_BIAS_GELU_BF16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = gelu_tanh_f(a[e]);
        } else if constexpr (EPI == BSI_EPI_BIAS_SILU_BF16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = silu_f(a[e]);
        }
        u32x2 w;
        w[0] = pack_bf16x2(a[0], a[1]);
        w[1] = pack_bf16x2(a[2], a[3]);
        *reinterpret_cast<u32x2*>(out + (size_t)m * ldo + c) = w;
    }
}

// fp32 counterpart (BSI_EPI_BIAS_F32): out[m][n] = bias[n] + sum over slabs, in slab order
__global__ __launch_bounds__(256) void splitk_finish_f32_kernel(const float* __restrict__ slabs, size_t slab_stride, int splits,
                                                                const float* __restrict__ bias, int M, int N, int ldo,
                                                                float* __restrict__ out) {
    const int n4 = N >> 2;
    const size_t total = (size_t)M * n4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / n4), c = (int)(i % n4) * 4;
        f32x4 a = bias ? *reinterpret_cast<const f32x4*>(bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < splits; ++sp) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(slabs + (size_t)sp * slab_stride + (size_t)m * N + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += v[e];
        }
        *reinterpret_cast<f32x4*>(out + (size_t)m * ldo + c) = a;
    }
}

// Per-sample GEMMs with an fp32 result (the adaLN MLP of a training step: M = images, N = 1024 or 6144, K = 1024 or 6144): 8-48
// tiles, each walking its whole K loop alone -- 52-71 us of pure latency per launch, 72 launches per step (3.7 ms of a 50 ms step at
// 64 images per GPU).  The slice count depends on K ONLY, so an output element is the same sum whatever M is (a batch and its shards
// stay bit-identical).
int splitk_plan_f32(int M, int N, int K) {
    if (M > 2048 || K < 1024 || N % 4 != 0) return 1;
    const int sp = K >= 4096 ? 8 : 4;
    if (K % (sp * 128) != 0) return 1;
    return sp;
}

// number of K slices for this problem (1 = do not split): only for few tiles, K long enough, slices of whole 128-column blocks
int splitk_plan(int M, int N, int K, int cus) {
    // K >= 2048 only: measured (tools/experiments/splitk_time.py) fc2 (K = 4096) 72 -> 28..40 us, but the K = 1024 GEMMs get slower
    // (22 -> 26..37 us): their K loop is already short and the fp32 slab round trip + finishing launch cost more than they save
    if (M <= 128 || M > 2048 || K < 2048 || K % 128 != 0 || N % 4 != 0) return 1;
    const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
    int best = 1;
    for (int sp = 2; sp <= 8; sp *= 2)
        if (K % (sp * 128) == 0 && K / sp >= 256 && tiles * sp <= cus) best = sp;
    return best;
}

template <int EPI>
int launch_splitk(const GemmParams& p0, int splits, void* workspace, hipStream_t s) {
    GemmParams p = p0;
    p.bias = nullptr;
    p.out = workspace;
    p.ldo = p.N;
    p.splits = splits;
    p.kslice = p.K / splits;
    p.slab_stride = (size_t)p.M * p.N;
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.gm = g_gm < p.tiles_m ? g_gm : p.tiles_m;
    if (p.gm < 1) p.gm = 1;
    const int nwg = p.tiles_m * p.tiles_n * splits;
    const int grid = nwg < compute_cus() ? nwg : compute_cus();
    const size_t lds = 4 * (size_t)512 * 64 + 32768;
    auto kern = gemm_bf16_pring_kernel<BSI_EPI_BIAS_F32>;
    set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, p);
    BSI_CHECK_LAUNCH("bsi_gemm_bf16_ws");
    const size_t total = (size_t)p.M * (p.N / 4);
    size_t g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    if constexpr (EPI == BSI_EPI_BIAS_F32)
        hipLaunchKernelGGL(splitk_finish_f32_kernel, dim3((int)g), dim3(256), 0, s, reinterpret_cast<const float*>(workspace), p.slab_stride,
                           splits, p0.bias, p.M, p.N, p0.ldo, reinterpret_cast<float*>(p0.out));
    else
        hipLaunchKernelGGL(splitk_finish_kernel<EPI>, dim3((int)g), dim3(256), 0, s, reinterpret_cast<const float*>(workspace), p.slab_stride,
                           splits, p0.bias, p.M, p.N, p0.ldo, reinterpret_cast<__bf16*>(p0.out));
    BSI_CHECK_LAUNCH("bsi_gemm_bf16_ws(finish)");
    return BSI_OK;
}

}  // namespace

extern "C" int bsi_gemm_set_variant(int v) {
    BSI_CHECK_ARG(v >= 0 && ((v & 0xff) == 12 || (v & 0xff) == 6),
                  "bsi_gemm_set_variant: unknown variant %d (12 = production, 6 = K = 32 ring; the other round-1 schedules live in "
                  "tools/experiments/gemm_variants.inc)", v & 0xff);
    g_variant = v & 0xff;
    g_gm = ((v >> 16) & 0xff) ? ((v >> 16) & 0xff) : 4;  // bits 16..23: band height of the tile walk
    return BSI_OK;
}

// does the MUL_GELUGRAD GEMM of this shape run the kernel whose epilogue can emit column sums (bsi_gemm_args::colsum_rows)?
bool bsi_gemm_emits_colsum(int M, int K) { return g_variant == 12 && M > 128 && K >= 128 && K % 64 == 0; }

// which arithmetic bsi_gemm_bf16_ws gives an output row of a plain bf16 epilogue of this shape when the persistent kernels may fill
// `cus` CUs: the split count (> 1) of the split-K path, else 1 for the large-M kernels (M > 128) and 0 for the small-M tile.  Two
// problems with the same N, K and plan compute every row with the same sums in the same order.
int bsi_gemm_ws_plan(int M, int N, int K, int cus) {
    const int sp = splitk_plan(M, N, K, cus);
    return sp > 1 ? sp : (M > 128 ? 1 : 0);
}

extern "C" int bsi_gemm_bf16(const bsi_gemm_args* a, bsi_stream_t stream) {
    BSI_CHECK_ARG(a != nullptr, "bsi_gemm_bf16: null args");
    BSI_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "bsi_gemm_bf16: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    BSI_CHECK_ARG(a->K % BK == 0, "bsi_gemm_bf16: K=%d must be a multiple of %d", a->K, BK);
    BSI_CHECK_ARG(a->N % 16 == 0, "bsi_gemm_bf16: N=%d must be a multiple of 16", a->N);
    BSI_CHECK_ARG(a->lda % 8 == 0 && a->ldw % 8 == 0 && a->lda >= a->K && a->ldw >= a->K,
                  "bsi_gemm_bf16: bad leading dimensions lda=%d ldw=%d", a->lda, a->ldw);
    BSI_CHECK_ARG(a->ldo % 8 == 0 && a->ldo >= a->N, "bsi_gemm_bf16: bad ldo=%d", a->ldo);
    BSI_CHECK_ARG(a->A && a->W && a->out, "bsi_gemm_bf16: null operand");
    GemmParams p{};
    p.A = reinterpret_cast<const __bf16*>(a->A);
    p.W = reinterpret_cast<const __bf16*>(a->W);
    p.bias = a->bias;
    p.out = a->out;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldw = a->ldw; p.ldo = a->ldo;
    p.gate = a->gate; p.gate_rows = a->gate_rows; p.gate_stride = a->gate_stride;
    p.tokens = a->tokens > 0 ? a->tokens : 1;
    p.pos = a->pos;
    p.aux = a->aux;
    p.out2 = a->out2;
    p.colsum = a->colsum_rows;
    BSI_CHECK_ARG(!a->colsum_rows || (a->epilogue == BSI_EPI_MUL_GELUGRAD_BF16 && bsi_gemm_emits_colsum(a->M, a->K)),
                  "bsi_gemm_bf16: colsum_rows is an output of the MUL_GELUGRAD epilogue of the K = 64 kernel (M > 128, K %% 64 == 0)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (a->epilogue) {
        case BSI_EPI_BIAS_F32: return launch_epi<BSI_EPI_BIAS_F32>(p, s);
        case BSI_EPI_BIAS_BF16: return launch_epi<BSI_EPI_BIAS_BF16>(p, s);
        case BSI_EPI_BIAS_GELU_BF16: return launch_epi<BSI_EPI_BIAS_GELU_BF16>(p, s);
        case BSI_EPI_BIAS_SILU_BF16: return launch_epi<BSI_EPI_BIAS_SILU_BF16>(p, s);
        case BSI_EPI_GATE_RESID:
            BSI_CHECK_ARG(a->gate && a->gate_rows > 0, "bsi_gemm_bf16: GATE_RESID needs gate");
            return launch_epi<BSI_EPI_GATE_RESID>(p, s);
        case BSI_EPI_BIAS_POS_F32:
            BSI_CHECK_ARG(a->pos && a->tokens > 0, "bsi_gemm_bf16: BIAS_POS needs pos/tokens");
            return launch_epi<BSI_EPI_BIAS_POS_F32>(p, s);
        case BSI_EPI_BIAS_GELU_DUAL:
            BSI_CHECK_ARG(a->out2, "bsi_gemm_bf16: GELU_DUAL needs out2");
            return launch_epi<BSI_EPI_BIAS_GELU_DUAL>(p, s);
        case BSI_EPI_MUL_GELUGRAD_BF16:
            BSI_CHECK_ARG(a->aux, "bsi_gemm_bf16: MUL_GELUGRAD needs aux");
            return launch_epi<BSI_EPI_MUL_GELUGRAD_BF16>(p, s);
        default:
            bsi_set_error("bsi_gemm_bf16: unknown epilogue %d", a->epilogue);
            return BSI_EINVAL;
    }
}

// `groups` GEMMs of one shape in ONE launch of the K = 32 ring kernel (fp32 output): operands, bias and output of group g lie g strides
// (bytes) behind those of `a`.  The per-sample adaLN matrices of the DiT blocks (M = images: 2 x N / 256 tiles each) fill the chip
// together; one at a time each needed split-K slabs and a finishing pass to do so.  Same kernel and K order whatever M is.
extern "C" int bsi_gemm_bf16_grouped(const bsi_gemm_args* a, int groups, size_t stride_a, size_t stride_w, size_t stride_bias, size_t stride_out,
                                     bsi_stream_t stream) {
    BSI_CHECK_ARG(a && a->A && a->W && a->out && groups >= 1 && groups <= 4096, "bsi_gemm_bf16_grouped: null operand or groups=%d", groups);
    BSI_CHECK_ARG(a->epilogue == BSI_EPI_BIAS_F32, "bsi_gemm_bf16_grouped: fp32 output with bias (BSI_EPI_BIAS_F32) only, got %d", a->epilogue);
    BSI_CHECK_ARG(a->M > 0 && a->N > 0 && a->K >= 96 && a->K % BK == 0 && a->N % 16 == 0, "bsi_gemm_bf16_grouped: M=%d N=%d K=%d (K >= 96, K %% %d == 0, N %% 16 == 0)",
                  a->M, a->N, a->K, BK);
    BSI_CHECK_ARG(a->lda % 8 == 0 && a->ldw % 8 == 0 && a->lda >= a->K && a->ldw >= a->K && a->ldo % 4 == 0 && a->ldo >= a->N,
                  "bsi_gemm_bf16_grouped: bad leading dimensions lda=%d ldw=%d ldo=%d", a->lda, a->ldw, a->ldo);
    BSI_CHECK_ARG(stride_a % 16 == 0 && stride_w % 16 == 0 && stride_bias % 16 == 0 && stride_out % 16 == 0, "bsi_gemm_bf16_grouped: strides must be multiples of 16 bytes");
    GemmParams p{};
    p.A = reinterpret_cast<const __bf16*>(a->A);
    p.W = reinterpret_cast<const __bf16*>(a->W);
    p.bias = a->bias;
    p.out = a->out;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldw = a->ldw; p.ldo = a->ldo;
    p.tokens = 1;
    p.groups = groups; p.g_a = stride_a; p.g_w = stride_w; p.g_bias = stride_bias; p.g_out = stride_out;
    p.tiles_m = (p.M + 255) / 256;
    p.tiles_n = (p.N + 255) / 256;
    p.gm = g_gm < p.tiles_m ? g_gm : p.tiles_m;
    if (p.gm < 1) p.gm = 1;
    const int nwg = p.tiles_m * p.tiles_n * (groups > 1 ? groups : 1);
    const int grid = nwg < compute_cus() ? nwg : compute_cus();
    const size_t lds = 4 * (size_t)512 * 64 + 32768;
    auto kern = gemm_bf16_pring_kernel<BSI_EPI_BIAS_F32>;
    set_max_lds(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, reinterpret_cast<hipStream_t>(stream), p);
    BSI_CHECK_LAUNCH("bsi_gemm_bf16_grouped");
    return BSI_OK;
}

extern "C" size_t bsi_gemm_splitk_workspace_bytes(int M, int N, int K) {
    const int sp = splitk_plan(M, N, K, device_cus());  // the most splits any CU reserve can ask for
    return sp > 1 ? (size_t)sp * (size_t)M * (size_t)N * sizeof(float) : 0;
}

extern "C" size_t bsi_gemm_splitk_f32_workspace_bytes(int M, int N, int K) {
    const int sp = splitk_plan_f32(M, N, K);
    return sp > 1 ? (size_t)sp * (size_t)M * (size_t)N * sizeof(float) : 0;
}

extern "C" int bsi_gemm_bf16_ws(const bsi_gemm_args* a, void* workspace, size_t workspace_bytes, bsi_stream_t stream) {
    // small-M latency path: split-K through the caller's workspace when the shape qualifies, the epilogue is a plain bf16 one
    // and the workspace is large enough; otherwise exactly bsi_gemm_bf16
    // the SAME argument contract as bsi_gemm_bf16 on both paths (round 1 skipped the N % 16 and K % 64 checks here)
    if (a && workspace && a->A && a->W && a->out && a->M > 0 && a->N > 0 && a->K > 0 && a->K % BK == 0 && a->N % 16 == 0 &&
        a->lda % 8 == 0 && a->ldw % 8 == 0 && a->lda >= a->K && a->ldw >= a->K && a->ldo % 4 == 0 && a->ldo >= a->N &&
        a->epilogue == BSI_EPI_BIAS_F32) {  // per-sample fp32 GEMMs (splitk_plan_f32)
        const int sp = splitk_plan_f32(a->M, a->N, a->K);
        if (sp > 1 && workspace_bytes >= (size_t)sp * (size_t)a->M * (size_t)a->N * sizeof(float)) {
            GemmParams p{};
            p.A = reinterpret_cast<const __bf16*>(a->A);
            p.W = reinterpret_cast<const __bf16*>(a->W);
            p.bias = a->bias;
            p.out = a->out;
            p.M = a->M; p.N = a->N; p.K = a->K;
            p.lda = a->lda; p.ldw = a->ldw; p.ldo = a->ldo;
            p.tokens = 1;
            return launch_splitk<BSI_EPI_BIAS_F32>(p, sp, workspace, reinterpret_cast<hipStream_t>(stream));
        }
    }
    if (a && workspace && a->A && a->W && a->out && a->M > 0 && a->N > 0 && a->K > 0 && a->K % BK == 0 && a->N % 16 == 0 &&
        a->lda % 8 == 0 && a->ldw % 8 == 0 && a->lda >= a->K && a->ldw >= a->K && a->ldo % 8 == 0 && a->ldo >= a->N &&
        (a->epilogue == BSI_EPI_BIAS_BF16 || a->epilogue == BSI_EPI_BIAS_GELU_BF16 || a->epilogue == BSI_EPI_BIAS_SILU_BF16)) {
        const int sp = splitk_plan(a->M, a->N, a->K, compute_cus());
        if (sp > 1 && workspace_bytes >= (size_t)sp * (size_t)a->M * (size_t)a->N * sizeof(float)) {
            GemmParams p{};
            p.A = reinterpret_cast<const __bf16*>(a->A);
            p.W = reinterpret_cast<const __bf16*>(a->W);
            p.bias = a->bias;
            p.out = a->out;
            p.M = a->M; p.N = a->N; p.K = a->K;
            p.lda = a->lda; p.ldw = a->ldw; p.ldo = a->ldo;
            p.tokens = 1;
            hipStream_t s = reinterpret_cast<hipStream_t>(stream);
            if (a->epilogue == BSI_EPI_BIAS_BF16) return launch_splitk<BSI_EPI_BIAS_BF16>(p, sp, workspace, s);
            if (a->epilogue == BSI_EPI_BIAS_GELU_BF16) return launch_splitk<BSI_EPI_BIAS_GELU_BF16>(p, sp, workspace, s);
            return launch_splitk<BSI_EPI_BIAS_SILU_BF16>(p, sp, workspace, s);
        }
    }
    return bsi_gemm_bf16(a, stream);
}

