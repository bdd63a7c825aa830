// Conv weight gradient on the bf16 matrix cores from PRE-SPLIT operand planes (bf16 engines, gfx950 / CDNA4):
//     dW[i][j = tap*Cin + ci] = sum_m dOut[m][i] * X[m shifted by tap][ci]
// Both operands are contracted over their ROW index m, so the MFMA operands (8 consecutive k = m per lane) are
// k-strided in memory.  The planes made by split_planes_kernel ([row][32-channel chunk][plane][32] bf16) are staged
// ROW-MAJOR into LDS with plain 16-byte copies (no conversion, half the bytes of an fp32 tile per plane) and the
// operands are fetched with gfx950's transposed LDS read ds_read_b64_tr_b16 (per 16-lane group a 4-row x 16-column
// block, delivered column-major: lane i gets column i, row e in element e — mapping checked on the device by
// tools/probes/tr_read_probe.hip).  LDS image per plane: [16 rows][128 columns] bf16 = 256-byte rows with the 16-byte
// chunk index XOR-swizzled by ((row&3)<<2 | (row>>2)&3), which keeps the transposed reads conflict-free.
// NT = 3: six MFMA terms of the exact hi+mid+lo split (fp32 accuracy); NT = 1: bf16 compute.
#include "pa2d_gemm_common.h"
#include "pa2d_bf16_split.h"      // s16x4 / s16x8 of the transposed LDS reads

struct MCPlanesParams {
    const void* PA; int chA;      // dOut planes, chA = 2C/32 chunks per row
    const void* PB; int chB;      // X planes, chB = Cin/32
    float* slab;
    int Mi, Nj, Mk, chunks_per_split, splits, H, W, Cin;
    unsigned a_bytes, b_bytes;
    int taps;                     // 9: columns are (tap, input channel) of a 3x3 conv; 1: plain dW = A^T . B (big kernel only)
    long long lda, ldb;           // F32SRC (128 x 128 kernel): PA / PB are fp32 row-major matrices [Mk][lda], [Mk][ldb]
    float* colsum;                // F32SRC, optional: [splits][Mi] per-split column sums of A (= a linear layer's bias gradient)
};

__device__ __forceinline__ unsigned img_off(int row, int ch) {       // byte offset inside one 4 KB plane image
    return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// 16x16x32 forms: the fragment of the wave's 16-column tile t_ in plane image pl_, from the lane's two addresses base_ for tile 0
// (tile t is `^ (t << 5)`).  Written on the builtins: through tr_frag the 256 x 256 kernel's address arithmetic changes.
#define MC16_FRAG(base_, t_, pl_)                                                                         \
    __builtin_bit_cast(bf16x8, __builtin_shufflevector(                                                   \
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + ((base_[0] ^ ((unsigned)(t_) << 5)) + (pl_) * PIMG))), \
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(smem + ((base_[1] ^ ((unsigned)(t_) << 5)) + (pl_) * PIMG))), \
        0, 1, 2, 3, 4, 5, 6, 7))

// KS = 16-row K-steps per LDS stage (one barrier per stage): 1 for NT = 3 (24 MFMAs per wave and barrier, 48 KB of LDS),
// 4 for NT = 1 (16 MFMAs per barrier instead of 4, 64 KB).
// F32SRC: plain dW = A^T . B of a linear layer straight from the fp32 operands (no tap shift): each thread loads the 8
// floats of its (row, 8-column piece) of both operands, splits them into the NT bf16 planes in registers and writes the
// same LDS plane images; the column sums of A (the bias gradient) are accumulated from the registers of column tile 0.
// MF16 (F32SRC, NT = 3, PA2D_MC_MFMA=16): v_mfma_f32_16x16x32_bf16 on 32-row K-steps read from two of THREE 16-row LDS slots
// (3 x 24 KB, still two workgroups per CU); the pipeline is the one of gemm_mc_planes_big_kernel's MF16 form below.
template <int NT, int KS, bool F32SRC = false, bool MF16 = false>
__global__ __launch_bounds__(256, 2) void gemm_mc_planes_kernel(const MCPlanesParams p) {
    constexpr int PIMG = 4096;                       // one plane image of one K-step: 16 rows x 256 B
    constexpr int STAGE = 2 * NT * KS * PIMG;        // A planes then B planes, KS sub-images each
    constexpr int NP = 2 * NT * KS;                  // 16-byte pieces per thread and stage
    __shared__ __attribute__((aligned(16))) unsigned char smem[(MF16 ? 3 : 2) * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_i = (p.Mi + 127) / 128, tiles_j = (p.Nj + 127) / 128;
    int tj, ti, split;
    MC_DECODE(p.splits, tiles_i, tiles_j, split, ti, tj)
    const int wm = wave >> 1, wn = wave & 1;
    const int total_chunks = (p.Mk + 15) / 16;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(total_chunks, c_begin + p.chunks_per_split);

    // the 128 columns of this tile are one tap and 4 consecutive 32-channel chunks of X
    const int j0 = tj * 128, tap = j0 / p.Cin, cb0 = (j0 - tap * p.Cin) >> 5, ca0 = (ti * 128) >> 5;
    const int tap_dy = tap / 3 - 1, tap_dx = tap - (tap / 3) * 3 - 1, tap_shift = tap_dy * p.W + tap_dx;
    const int HW = p.H * p.W;

    const __amdgpu_buffer_rsrc_t ra_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.PA), 0, p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.PB), 0, p.b_bytes, 0x00020000);

    // staging assignment: piece id q = tid + 256*s in [0, 512*NT): operand, row, chunk, plane, 16-byte piece
    int s_row[NP];
    unsigned s_goff[NP], s_lds[NP];
    bool s_isb[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        const int q = tid + 256 * s;
        const int op = q / (256 * NT * KS), r = q - op * (256 * NT * KS);
        const int row = r / (16 * NT), rr = r - row * (16 * NT);          // row in [0, 16*KS)
        const int c = rr / (4 * NT), pp = rr - c * (4 * NT);
        const int plane = pp >> 2, piece = pp & 3;
        s_row[s] = row;
        s_isb[s] = op != 0;
        s_goff[s] = (unsigned)((((op ? cb0 : ca0) + c) * NT + plane) * 64 + piece * 16);
        s_lds[s] = (unsigned)(((op * NT + plane) * KS + (row >> 4)) * PIMG) + img_off(row & 15, c * 4 + piece);
    }
    u32x4 rg[F32SRC ? 4 * KS : NP];
    // F32SRC staging: thread = (row, 8-column piece) of both operands
    const int frow = tid >> 4, fc8 = tid & 15;
    const unsigned flds = img_off(frow, fc8);
    const bool fok_a = ti * 128 + fc8 * 8 < p.Mi, fok_b = tj * 128 + fc8 * 8 < p.Nj;
    const unsigned fcol_a = (unsigned)(ti * 128 + fc8 * 8) * 4u, fcol_b = (unsigned)(tj * 128 + fc8 * 8) * 4u;
    const unsigned fpitch_a = (unsigned)p.lda * 4u, fpitch_b = (unsigned)p.ldb * 4u;
    float cs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[e] = 0.f;
#define MP_LOAD(c_)                                                                                       \
    if constexpr (F32SRC) {                                                                               \
        _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                               \
            const int m_ = ((c_) + ks) * 16 + frow;                                                       \
            const bool okr_ = m_ < p.Mk && (c_) + ks < c_end;                                             \
            const unsigned oa_ = (okr_ && fok_a) ? (unsigned)m_ * fpitch_a + fcol_a : OOB_OFF;            \
            const unsigned ob_ = (okr_ && fok_b) ? (unsigned)m_ * fpitch_b + fcol_b : OOB_OFF;            \
            rg[ks * 4 + 0] = __builtin_amdgcn_raw_buffer_load_b128(ra_rsrc, oa_, 0, 0);                   \
            rg[ks * 4 + 1] = __builtin_amdgcn_raw_buffer_load_b128(ra_rsrc, oa_ == OOB_OFF ? OOB_OFF : oa_ + 16u, 0, 0); \
            rg[ks * 4 + 2] = __builtin_amdgcn_raw_buffer_load_b128(rb_rsrc, ob_, 0, 0);                   \
            rg[ks * 4 + 3] = __builtin_amdgcn_raw_buffer_load_b128(rb_rsrc, ob_ == OOB_OFF ? OOB_OFF : ob_ + 16u, 0, 0); \
        }                                                                                                 \
    } else {                                                                                              \
        const int m0_ = (c_) * 16;                                                                        \
        _Pragma("unroll") for (int s = 0; s < NP; ++s) {                                                  \
            const int m_ = m0_ + s_row[s];                                                                \
            bool ok_ = m_ < p.Mk && (KS == 1 || (c_) + (s_row[s] >> 4) < c_end);   /* next split's rows stay out */ \
            int mm_ = m_;                                                                                 \
            if (s_isb[s]) {                                                                               \
                const int n_ = m_ % HW;                                                                   \
                const int y_ = n_ / p.W, x_ = n_ - y_ * p.W;                                              \
                ok_ = ok_ && (unsigned)(y_ + tap_dy) < (unsigned)p.H && (unsigned)(x_ + tap_dx) < (unsigned)p.W; \
                mm_ = m_ + tap_shift;                                                                     \
            }                                                                                             \
            const unsigned rowb_ = (unsigned)mm_ * (unsigned)((s_isb[s] ? p.chB : p.chA) * NT * 64);      \
            rg[s] = s_isb[s] ? __builtin_amdgcn_raw_buffer_load_b128(rb_rsrc, ok_ ? rowb_ + s_goff[s] : OOB_OFF, 0, 0) \
                             : __builtin_amdgcn_raw_buffer_load_b128(ra_rsrc, ok_ ? rowb_ + s_goff[s] : OOB_OFF, 0, 0); \
        }                                                                                                 \
    }
#define MP_STORE(buf_)                                                                                    \
    if constexpr (F32SRC) {                                                                               \
        _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) _Pragma("unroll") for (int op = 0; op < 2; ++op) { \
            bf16x8 pk_[NT];                                                                               \
            MC_SPLIT_ROW8(NT, rg[ks * 4 + op * 2], rg[ks * 4 + op * 2 + 1], op == 0 && do_cs, cs, pk_)   \
            unsigned char* d_ = smem + (buf_) * STAGE + flds;                                             \
            _Pragma("unroll") for (int pl = 0; pl < NT; ++pl)                                             \
                *reinterpret_cast<bf16x8*>(d_ + ((op * NT + pl) * KS + ks) * PIMG) = pk_[pl];             \
        }                                                                                                 \
    } else {                                                                                              \
        _Pragma("unroll") for (int s = 0; s < NP; ++s)                                                    \
            *reinterpret_cast<u32x4*>(smem + (buf_) * STAGE + s_lds[s]) = rg[s];                          \
    }
    const bool do_cs = F32SRC && p.colsum != nullptr && tj == 0;

    if constexpr (MF16) {
        // see gemm_mc_planes_big_kernel: lane groups 0 / 1 read rows 0-7 / 8-15 of the step's first slot, groups 2 / 3 of its
        // second; B (the layer input) is the MFMA's A operand, so an accumulator quad is four consecutive columns of dW
        static_assert(NT == 3 && KS == 1 && F32SRC, "the 16x16x32 form is written for the split engine's linear weight gradient");
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kq = lane >> 4, q4 = (lane & 15) >> 2, pq = lane & 3;
        unsigned fa[2], fb[2];                            // 16-column tile 0 of the wave; tile t is `^ (t << 5)`
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 8 * (kq & 1) + 4 * r + q4;
            fa[r] = img_off(row, wm * 8 + (pq >> 1)) + 8u * (pq & 1);
            fb[r] = img_off(row, wn * 8 + (pq >> 1)) + 8u * (pq & 1);
        }
#define MP16_MMA(ib_, AF) _Pragma("unroll") for (int j = 0; j < 4; ++j) split_terms(AF, xf[j], acc[ib_][j]);
        // staging in two parts: MP16_CONVERT splits the fp32 registers into the bf16 planes (and adds to the column sums) while
        // the other waves still multiply, MP16_WRITE is the six 16-byte LDS stores alone -> only those sit between the barriers
        bf16x8 pk[2][NT];
#define MP16_CONVERT()                                                                                    \
    _Pragma("unroll") for (int op = 0; op < 2; ++op) MC_SPLIT_ROW8(NT, rg[op * 2], rg[op * 2 + 1], op == 0 && do_cs, cs, pk[op])
#define MP16_WRITE(buf_)                                                                                  \
    _Pragma("unroll") for (int op = 0; op < 2; ++op) _Pragma("unroll") for (int pl = 0; pl < NT; ++pl)    \
        *reinterpret_cast<bf16x8*>(smem + (buf_) * STAGE + flds + (op * NT + pl) * PIMG) = pk[op][pl];
        const int nst = c_end - c_begin, steps = (nst + 1) >> 1;
        if (nst > 0) {
            MP_LOAD(c_begin)
            MP16_CONVERT()
            MP16_WRITE(0)
            MP_LOAD(c_begin + 1)
            MP16_CONVERT()
            MP16_WRITE(1)
            if (steps > 1) { MP_LOAD(c_begin + 2) }
        }
        __syncthreads();
        // step k (stages 2k, 2k+1 in slots P, Q; R free; the registers hold stage 2k+2 in flight): tile 0 | convert and write
        // stage 2k+2 to R, load 2k+3 | tiles 1, 2 | convert 2k+3, load 2k+4 | barrier | write P | tile 3 | barrier: every load
        // has half a step to land, as in the 32x32x16 form.  Each stage is converted exactly once (column sums).
        int sp = 0, sq = 1, sr = 2;
        for (int k = 0; k < steps; ++k) {
            const bool has_next = k + 1 < steps;          // workgroup-uniform
            const unsigned lo = (unsigned)((kq >> 1) ? sq : sp) * (unsigned)STAGE;     // this lane group's slot (a multiple of 4 KB)
            const unsigned ua[2] = {fa[0] + lo, fa[1] + lo};
            const unsigned ub[2] = {fb[0] + lo + NT * PIMG, fb[1] + lo + NT * PIMG};
            bf16x8 xf[4][NT];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int pl = 0; pl < NT; ++pl) xf[j][pl] = MC16_FRAG(ub, j, pl);
            bf16x8 afc[NT], afn[NT];                      // A fragments one 16-row tile ahead of their MFMAs
#pragma unroll
            for (int pl = 0; pl < NT; ++pl) afc[pl] = MC16_FRAG(ua, 0, pl);
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                if (ib < 3) {
#pragma unroll
                    for (int pl = 0; pl < NT; ++pl) afn[pl] = MC16_FRAG(ua, ib + 1, pl);
                }
                if (ib == 1 && has_next) {
                    MP16_CONVERT()
                    MP16_WRITE(sr)
                    MP_LOAD(c_begin + 2 * k + 3)
                }
                if (ib == 3) {       // every LDS read of the step is done: P is free; the last tile's MFMAs cover its refill
                    if (has_next) {
                        MP16_CONVERT()
                        if (k + 2 < steps) { MP_LOAD(c_begin + 2 * k + 4) }
                    }
                    __syncthreads();
                    if (has_next) { MP16_WRITE(sp) }
                }
                MP16_MMA(ib, afc)
#pragma unroll
                for (int pl = 0; pl < NT; ++pl) afc[pl] = afn[pl];
            }
            __syncthreads();
            const int t = sp;
            sp = sr;
            sr = sq;
            sq = t;
        }
#undef MP16_CONVERT
#undef MP16_WRITE
#undef MP16_MMA
        if (do_cs) {       // as below: LDS is free after the last barrier
            float* sm = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[frow * 128 + fc8 * 8 + e] = cs[e];
            mc_colsum_reduce<128, 16>(sm, tid, ti, split, p.Mi, p.colsum);
        }
        // accumulator quad r = 0..3 of lane l: dW row ti*128 + wm*64 + ib*16 + (l & 15), columns tj*128 + wn*64 + j*16 +
        // 4*(l >> 4) + r (Nj % 4 == 0, checked by the launcher: a quad is inside or outside as a whole)
        float* out = p.slab + (size_t)split * p.Mi * p.Nj;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = tj * 128 + wn * 64 + j * 16 + 4 * kq;
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const int row = ti * 128 + wm * 64 + ib * 16 + (lane & 15);
                if (row < p.Mi && col < p.Nj) *reinterpret_cast<f32x4*>(out + (size_t)row * p.Nj + col) = acc[ib][j];
            }
        }
        return;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addresses of this lane: group g = lane>>4 covers columns 16*(g&1).. of a 32-wide tile and
    // rows 8*(g>>1)..; lane 4q+pq of the group supplies row q, columns 4pq..4pq+3 (8 bytes)
    const int g = lane >> 4, q4 = (lane & 15) >> 2, pq = lane & 3;
    unsigned fa[2][2], fb[2][2];                      // [tile][read r]: byte offset inside a plane image
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 8 * (g >> 1) + 4 * r + q4;
            const int cha = ((wm * 64 + t * 32) >> 3) + 2 * (g & 1) + (pq >> 1);
            const int chb = ((wn * 64 + t * 32) >> 3) + 2 * (g & 1) + (pq >> 1);
            fa[t][r] = img_off(row, cha) + 8u * (pq & 1);
            fb[t][r] = img_off(row, chb) + 8u * (pq & 1);
        }

    if (c_begin < c_end) {
        MP_LOAD(c_begin)
        MP_STORE(0)
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; c += KS) {
        const int buf = ((c - c_begin) / KS) & 1;
        if (c + KS < c_end) { MP_LOAD(c + KS) }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
        const unsigned char* st = smem + buf * STAGE + ks * PIMG;
        bf16x8 af[2][NT], bf[2][NT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pl = 0; pl < NT; ++pl) {
                af[t][pl] = tr_frag(st + pl * KS * PIMG, fa[t][0], fa[t][1]);
                bf[t][pl] = tr_frag(st + (NT + pl) * KS * PIMG, fb[t][0], fb[t][1]);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) split_terms(af[i], bf[j], acc[i][j]);
        }
        if (c + KS < c_end) { MP_STORE(buf ^ 1) }
        __syncthreads();
    }
#undef MP_LOAD
#undef MP_STORE

    if constexpr (F32SRC) {
        if (do_cs) {       // the 16 row-threads of a column piece add up through LDS (free after the last barrier)
            float* sm = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[frow * 128 + fc8 * 8 + e] = cs[e];
            mc_colsum_reduce<128, 16>(sm, tid, ti, split, p.Mi, p.colsum);
        }
    }
    float* out = p.slab + (size_t)split * p.Mi * p.Nj;
    const int col0 = tj * 128 + wn * 64 + (lane & 31);
    const int row0 = ti * 128 + wm * 64 + 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + i * 32 + (r & 3) + 8 * (r >> 2);
                if (!F32SRC || (row < p.Mi && col0 + j * 32 < p.Nj)) out[(size_t)row * p.Nj + col0 + j * 32] = acc[i][j][r];
            }
}

// =============================================================================================================
// 256 x 256 tile, 8 waves (2 per SIMD), every wave stages AND multiplies: the 128 x 128 kernel above moves 24 KB per 24
// MFMAs per wave and sits at the ~70 GB/s per CU at which L2 feeds a CU (1.75 ms per launch at the bench shape, MFMA
// floor 0.74).  Here a workgroup owns 256 dOut channels x 256 columns (= 8 groups of 32 input channels, each group
// with its own tap, so any Cin % 32 == 0 works) and each wave a 128 x 64 quarter-strip (4 x 2 MFMA tiles): 48 KB per
// K-step of 16 pixel rows for 8 x 48 MFMAs, i.e. HALF the staging bytes and 3/4 of the LDS fragment reads per MFMA,
// and 48 MFMAs between barriers instead of 24.  LDS: 2 stages x NT x (8 KB dOut image + 8 KB X image) = 96 KB, one
// workgroup per CU.  The launch is ONE round of <= 256 workgroups (tiles x splits); workgroups are numbered so that each
// XCD (blockIdx & 7) owns a contiguous range of (split, i-tile, j-tile): the 9+ workgroups that re-read the same dOut
// rows and the same X rows (at different tap shifts) sit behind one L2.
// MF16 (NT = 3; PA2D_MC_MFMA=32 turns it off): v_mfma_f32_16x16x32_bf16 on 32-row K-steps read from two of THREE 16-row LDS slots (144 KB);
// same tile, plane images, transposed reads and bytes per MAC (see the branch below).
// DMA (MF16 only; PA2D_MC_DMA=0 turns it off): the slots are filled by buffer_load_dwordx4 ... lds, global -> LDS with no
// staging registers and no ds_write.  CHAIN (on top of DMA; PA2D_MC_CHAIN): the six terms of an accumulator issue back to back.
#ifndef MB_MID
#define MB_MID 5      // DMA: the dOut tile in front of whose MFMAs the slot-freeing barrier of a step sits (7 = where register staging has it)
#endif
template <int NT, int KS, bool MF16 = false, bool DMA = false, bool CHAIN = false>
__global__ __launch_bounds__(512, 1) void gemm_mc_planes_big_kernel(const MCPlanesParams p, const int per_xcd) {
    constexpr int PIMG = 8192;                       // one plane image of one K-step: 16 rows x 512 B (256 bf16 columns)
    constexpr int STAGE = 2 * NT * KS * PIMG;        // dOut planes then X planes
    constexpr int NP = (2 * NT * KS * 512) / 512;    // 16-byte pieces per thread and stage (16 rows x 32 pieces x NT x 2 / 512)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_i = (p.Mi + 255) / 256, tiles_j = (p.Nj + 255) / 256;
    const int tiles = tiles_i * tiles_j;
    const int lin = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);      // XCD-contiguous numbering
    if ((int)(blockIdx.x >> 3) >= per_xcd || lin >= tiles * p.splits) return;
    const int split = lin / tiles, t_ = lin - split * tiles;
    const int ti = t_ / tiles_j, tj = t_ - ti * tiles_j;
    const int wm = wave >> 2, wn = wave & 3;         // 2 x 4 waves: 128 rows x 64 columns each
    const int total_chunks = (p.Mk + 15) / 16;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(total_chunks, c_begin + p.chunks_per_split);
    const int HW = p.taps == 1 ? 1 : p.H * p.W;

    const __amdgpu_buffer_rsrc_t ra_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.PA), 0, p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.PB), 0, p.b_bytes, 0x00020000);

    // staging assignment: the 512 threads cover ONE plane image of ONE 16-row K-step (16 rows x 32 pieces of 16 bytes);
    // piece s of a thread = (operand, plane, k-step) of the same (row, column group c, piece) -> the metadata is per
    // thread, not per piece (a second register set for a 2-stage-deep prefetch was tried: 256 VGPRs + 160 spilled)
    // DMA: one wave-instruction writes 64 x 16 bytes CONTIGUOUSLY (wave w = rows 2w, 2w+1 of an image, thread t at byte 16 t),
    // so the row swizzle moves to the global side: thread t fetches the chunk that belongs at linear position t & 31 of its
    // row, i.e. chunk (t & 31) ^ swizzle(row) -- the image the transposed reads see is byte for byte the same
    static_assert(!DMA || MF16, "LDS-DMA staging is written for the 16x16x32 pipeline");
    static_assert(!CHAIN || DMA, "the chained issue order needs the registers that DMA staging frees");
    const int row16 = tid >> 5;
    const int lchunk = DMA ? (tid & 31) ^ (((row16 & 3) << 2) | ((row16 >> 2) & 3)) : (tid & 31);
    const int cgrp = lchunk >> 2, piece = lchunk & 3;
    const bool colok_a = ti * 256 + cgrp * 32 < p.Mi;
    const unsigned goff_a = (unsigned)((((ti * 256) >> 5) + cgrp) * NT * 64 + piece * 16);
    const int jc = tj * 256 + cgrp * 32;             // X: column group = one tap, one 32-channel chunk
    const int tap = p.taps == 1 ? 4 : jc / p.Cin;    // plain GEMM: the centre tap (no shift)
    const bool colok_b = jc < p.Nj;
    const unsigned goff_b = (unsigned)((p.taps == 1 ? (jc >> 5) : ((jc - tap * p.Cin) >> 5)) * NT * 64 + piece * 16);
    const int tap_dy = tap / 3 - 1, tap_dx = tap - (tap / 3) * 3 - 1, tap_shift = tap_dy * p.W + tap_dx;
    const unsigned pitch_a = (unsigned)(p.chA * NT * 64), pitch_b = (unsigned)(p.chB * NT * 64);
    const unsigned lds_off = 512u * row16 + 16u * ((unsigned)(cgrp * 4 + piece) ^ (unsigned)(((row16 & 3) << 2) | ((row16 >> 2) & 3)));
#define MB_LOAD(c_, RG)                                                                                   \
    {                                                                                                     \
        _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                               \
            const int m_ = ((c_) + ks) * 16 + row16;                                                      \
            const bool okr_ = m_ < p.Mk && (c_) + ks < c_end;      /* next split's rows stay out */       \
            bool okb_ = okr_ && colok_b;                                                                  \
            int mm_ = m_;                                                                                 \
            if (p.taps != 1) {      /* (ly, lx) = pixel of row m_ in its image, advanced 16 rows per K-step */ \
                okb_ = okb_ && (unsigned)(ly + tap_dy) < (unsigned)p.H && (unsigned)(lx + tap_dx) < (unsigned)p.W; \
                mm_ = m_ + tap_shift;                                                                     \
                lx += 16;                                                                                 \
                while (lx >= p.W) { lx -= p.W; ++ly; }                                                    \
                while (ly >= p.H) ly -= p.H;                                                              \
            }                                                                                             \
            const unsigned oa_ = (okr_ && colok_a) ? (unsigned)m_ * pitch_a + goff_a : OOB_OFF;           \
            const unsigned ob_ = okb_ ? (unsigned)mm_ * pitch_b + goff_b : OOB_OFF;                       \
            _Pragma("unroll") for (int pl = 0; pl < NT; ++pl) {                                           \
                RG[pl * KS + ks] = __builtin_amdgcn_raw_buffer_load_b128(ra_rsrc, oa_ == OOB_OFF ? OOB_OFF : oa_ + pl * 64u, 0, 0); \
                RG[(NT + pl) * KS + ks] = __builtin_amdgcn_raw_buffer_load_b128(rb_rsrc, ob_ == OOB_OFF ? OOB_OFF : ob_ + pl * 64u, 0, 0); \
            }                                                                                             \
        }                                                                                                 \
    }
#define MB_STORE(buf_, RG)                                                                                \
    {                                                                                                     \
        _Pragma("unroll") for (int s = 0; s < NP; ++s)                                                    \
            *reinterpret_cast<u32x4*>(smem + (buf_) * STAGE + s * PIMG + lds_off) = RG[s];                \
    }
    // stage c_ straight into slot buf_ (KS = 1).  Same offsets and the same range check as MB_LOAD: rows outside the image,
    // past c_end or past Mk arrive as zeros; the wave's LDS base goes through M0, the lanes follow at 16 bytes each
#define MB_DMA(c_, buf_)                                                                                  \
    {                                                                                                     \
        const int m_ = (c_) * 16 + row16;                                                                 \
        const bool okr_ = m_ < p.Mk && (c_) < c_end;                                                      \
        bool okb_ = okr_ && colok_b;                                                                      \
        int mm_ = m_;                                                                                     \
        if (p.taps != 1) {                                                                                \
            okb_ = okb_ && (unsigned)(ly + tap_dy) < (unsigned)p.H && (unsigned)(lx + tap_dx) < (unsigned)p.W; \
            mm_ = m_ + tap_shift;                                                                         \
            lx += 16;                                                                                     \
            while (lx >= p.W) { lx -= p.W; ++ly; }                                                        \
            while (ly >= p.H) ly -= p.H;                                                                  \
        }                                                                                                 \
        const unsigned oa_ = (okr_ && colok_a) ? (unsigned)m_ * pitch_a + goff_a : OOB_OFF;               \
        const unsigned ob_ = okb_ ? (unsigned)mm_ * pitch_b + goff_b : OOB_OFF;                           \
        const unsigned va_[NT] = {oa_, oa_ == OOB_OFF ? OOB_OFF : oa_ + 64u, oa_ == OOB_OFF ? OOB_OFF : oa_ + 128u}; \
        const unsigned vb_[NT] = {ob_, ob_ == OOB_OFF ? OOB_OFF : ob_ + 64u, ob_ == OOB_OFF ? OOB_OFF : ob_ + 128u}; \
        unsigned keep_;                                                                                   \
        asm volatile(MB_DMA_ASM                                                                           \
                     : "=&s"(keep_)                                                                       \
                     : "s"(lds_base + (unsigned)(buf_) * (unsigned)STAGE), "s"(dma_ra), "s"(dma_rb),      \
                       "v"(va_[0]), "v"(va_[1]), "v"(va_[2]), "v"(vb_[0]), "v"(vb_[1]), "v"(vb_[2])       \
                     : "memory", "scc");                                                                  \
    }
    // The six images of a slot are 8 KB apart: M0 steps through them.  The compiler neither counts these loads nor knows that
    // they write LDS (told so, through the builtin, it drains them with vmcnt(0) in front of the next fragment read): MB_DMA_WAIT
    // in front of a barrier is the wait.  M0 is the compiler's: saved and restored inside the statement.
#define MB_DMA_ASM                                                                                        \
    "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"                                      \
    "buffer_load_dwordx4 %4, %2, 0 offen lds\n\ts_add_u32 m0, m0, 0x2000\n\ts_nop 0\n\t"                  \
    "buffer_load_dwordx4 %5, %2, 0 offen lds\n\ts_add_u32 m0, m0, 0x2000\n\ts_nop 0\n\t"                  \
    "buffer_load_dwordx4 %6, %2, 0 offen lds\n\ts_add_u32 m0, m0, 0x2000\n\ts_nop 0\n\t"                  \
    "buffer_load_dwordx4 %7, %3, 0 offen lds\n\ts_add_u32 m0, m0, 0x2000\n\ts_nop 0\n\t"                  \
    "buffer_load_dwordx4 %8, %3, 0 offen lds\n\ts_add_u32 m0, m0, 0x2000\n\ts_nop 0\n\t"                  \
    "buffer_load_dwordx4 %9, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
#define MB_DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
    static_assert(!DMA || (NT == 3 && PIMG == 0x2000), "MB_DMA_ASM is written out for six 8 KB images");
    typedef __attribute__((address_space(3))) unsigned char lds_char;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_char*)smem + (unsigned)__builtin_amdgcn_readfirstlane(wave) * 1024u;
    const u32x4 dma_ra = {(unsigned)(uintptr_t)p.PA, (unsigned)((uintptr_t)p.PA >> 32) & 0xFFFFu, p.a_bytes, 0x00020000u};
    const u32x4 dma_rb = {(unsigned)(uintptr_t)p.PB, (unsigned)((uintptr_t)p.PB >> 32) & 0xFFFFu, p.b_bytes, 0x00020000u};
    u32x4 rg0[DMA ? 1 : NP];
    // pixel coordinates of this thread's row of the NEXT K-step to be loaded: two integer divisions once, not per K-step
    // (the loads walk the rows in order, 16 per K-step; PMC before: 2.4 vector instructions per MFMA, most of them these)
    int ly = 0, lx = 0;
    if (p.taps != 1) {
        const int n0 = (c_begin * 16 + row16) % HW;
        ly = n0 / p.W;
        lx = n0 - ly * p.W;
    }

    if constexpr (MF16) {
        // v_mfma_f32_16x16x32_bf16 on REAL 32-row K-steps: LDS holds THREE 16-row slots (3 x 48 KB), a K-step reads two of
        // them.  Lane group kq = lane>>4 of a 16x16x32 operand holds k = 8kq .. 8kq+7, so groups 0 / 1 take rows 0-7 / 8-15
        // of the step's first slot and groups 2 / 3 the same rows of its second slot: the same two transposed reads per
        // fragment and the same bytes per MAC as the 32x32x16 form, no duplicated data.  X is the A operand (rows = columns
        // j of dW), so a lane's accumulator quad is four consecutive j of one dOut channel: 16-byte stores.
        // Pipeline of step k (stages 2k, 2k+1 in slots P, Q; slot R free; the register set holds stage 2k+2 in flight):
        //   MFMAs of dOut tiles 0-3 | store the registers to R, load stage 2k+3 | tiles 4-6, tile 7's fragments | barrier |
        //   store the registers to P, load stage 2k+4 | MFMAs of tile 7 | barrier;  next step: (R, P), Q free.
        // A split with an odd chunk count ends on a half-empty step: the rows past c_end load as zeros (MB_LOAD).
        static_assert(NT == 3 && KS == 1, "the 16x16x32 form is written for the split engine");
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kq = lane >> 4, q4 = (lane & 15) >> 2, pq = lane & 3;
        // byte offset of this lane's address in a plane image for 16-column tile 0 of the wave; tile t is `^ (t << 5)`:
        // the tile index sits in chunk bits 1..3, which the row swizzle XORs and nothing else touches
        unsigned fa[2], fb[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 8 * (kq & 1) + 4 * r + q4;
            const unsigned swz = (unsigned)(((row & 3) << 2) | ((row >> 2) & 3));
            fa[r] = 512u * row + 16u * ((unsigned)(wm * 16 + (pq >> 1)) ^ swz) + 8u * (pq & 1);
            fb[r] = 512u * row + 16u * ((unsigned)(wn * 8 + (pq >> 1)) ^ swz) + 8u * (pq & 1);
        }
        // CHAIN: left alone the compiler interleaves the four accumulators of a row block term by term; a pin behind each
        // accumulator keeps its six terms together (same per-accumulator order: the outputs do not change by a bit)
#define MB16_MMA(ib_, AF)                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
        split_terms(AF, xf[j], acc[ib_][j]);                                                              \
        if constexpr (CHAIN) MB16_CHAIN_PIN(j)                                                            \
    }
#define MB16_CHAIN_PIN(j_) __builtin_amdgcn_sched_barrier(0);
        const int nst = c_end - c_begin, steps = (nst + 1) >> 1;
        // DMA pipeline of step k (no register set; M = MB_MID): tile 0 | DMA stage 2k+2 to R | tiles 1..M-1, fragments of tiles
        //   M..7 | barrier | DMA stage 2k+3 to P | MFMAs of tiles M..7 | vmcnt(0) | barrier: every wave has its own pieces of both
        //   slots in LDS before the barrier that publishes them, and no fragment read of R or P lies between a DMA and that
        //   barrier.  M = 5: 1.07 ms where M = 7 runs 1.21 and register staging 1.19.
        if (nst > 0) {
            if constexpr (DMA) {
                MB_DMA(c_begin, 0)
                MB_DMA(c_begin + 1, 1)
                MB_DMA_WAIT();
            } else {
                MB_LOAD(c_begin, rg0)
                MB_STORE(0, rg0)
                MB_LOAD(c_begin + 1, rg0)
                MB_STORE(1, rg0)
                if (steps > 1) MB_LOAD(c_begin + 2, rg0)
            }
        }
        __syncthreads();
        int sp = 0, sq = 1, sr = 2;
        for (int k = 0; k < steps; ++k) {
            const unsigned lo = (unsigned)((kq >> 1) ? sq : sp) * (unsigned)STAGE;     // this lane group's slot
            // slot offsets are multiples of 8 KB: adding them first commutes with the tile XOR of bits 5..7
            const unsigned ua[2] = {fa[0] + lo, fa[1] + lo};
            const unsigned ub[2] = {fb[0] + lo + NT * PIMG, fb[1] + lo + NT * PIMG};
            bf16x8 xf[4][NT];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int pl = 0; pl < NT; ++pl) xf[j][pl] = MC16_FRAG(ub, j, pl);
            // dOut fragments one 16-row tile ahead of their MFMAs.  Stores and loads past the last step are harmless (free
            // slots, out-of-range offsets) and keep the loop body free of branches.
            if constexpr (DMA) {
                // the DMA into P has no registers to land in while P is still read: it starts at the barrier that frees P and
                // must be in LDS at the end of the step.  So the barrier moves up to tile MB_MID, and the fragments of the
                // tiles from there on are read before it, together with tile MB_MID's
                bf16x8 af[8][NT];
#pragma unroll
                for (int pl = 0; pl < NT; ++pl) af[0][pl] = MC16_FRAG(ua, 0, pl);
#pragma unroll
                for (int ib = 0; ib < 8; ++ib) {
#pragma unroll
                    for (int t = 1; t < 8; ++t)
                        if (ib + 1 == (t < MB_MID ? t : MB_MID)) {
#pragma unroll
                            for (int pl = 0; pl < NT; ++pl) af[t][pl] = MC16_FRAG(ua, t, pl);
                        }
                    if (ib == 1) MB_DMA(c_begin + 2 * k + 2, sr)
                    if (ib == MB_MID) {      // every LDS read of the step is done: P is free
                        __syncthreads();
                        MB_DMA(c_begin + 2 * k + 3, sp)
                    }
                    MB16_MMA(ib, af[ib])
                }
                MB_DMA_WAIT();
            } else {
            bf16x8 afc[NT], afn[NT];
#pragma unroll
            for (int pl = 0; pl < NT; ++pl) afc[pl] = MC16_FRAG(ua, 0, pl);
#pragma unroll
            for (int ib = 0; ib < 8; ++ib) {
                if (ib < 7) {
#pragma unroll
                    for (int pl = 0; pl < NT; ++pl) afn[pl] = MC16_FRAG(ua, ib + 1, pl);
                }
                if (ib == 4) {
                    MB_STORE(sr, rg0)
                    MB_LOAD(c_begin + 2 * k + 3, rg0)
                }
                if (ib == 7) {       // every LDS read of the step is done: P is free; the last tile's MFMAs cover its refill
                    __syncthreads();
                    MB_STORE(sp, rg0)
                    MB_LOAD(c_begin + 2 * k + 4, rg0)
                }
                MB16_MMA(ib, afc)
#pragma unroll
                for (int pl = 0; pl < NT; ++pl) afc[pl] = afn[pl];
            }
            }
            __syncthreads();
            const int t = sp;
            sp = sr;
            sr = sq;
            sq = t;
        }
#undef MB16_MMA
#undef MB16_CHAIN_PIN
        // accumulator quad r = 0..3 of lane l: dW row (dOut channel) ti*256 + wm*128 + ib*16 + (l & 15), columns
        // tj*256 + wn*64 + j*16 + 4*(l >> 4) + r (Nj % 32 == 0: a quad is inside or outside as a whole)
        float* out = p.slab + (size_t)split * p.Mi * p.Nj;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = tj * 256 + wn * 64 + j * 16 + 4 * kq;
            if (col >= p.Nj) continue;
#pragma unroll
            for (int ib = 0; ib < 8; ++ib) {
                const int row = ti * 256 + wm * 128 + ib * 16 + (lane & 15);
                if (row < p.Mi) *reinterpret_cast<f32x4*>(out + (size_t)row * p.Nj + col) = acc[ib][j];
            }
        }
        return;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addresses (see the 128 x 128 kernel): group g = lane>>4 covers columns 16*(g&1).. of a 32-wide tile
    // and rows 8*(g>>1)..; lane 4q+pq of the group supplies row q, columns 4pq..4pq+3 (8 bytes)
    const int g = lane >> 4, q4 = (lane & 15) >> 2, pq = lane & 3;
    unsigned fa[4][2], fb[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 8 * (g >> 1) + 4 * r + q4;
        const unsigned swz = (unsigned)(((row & 3) << 2) | ((row >> 2) & 3));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cha = ((wm * 128 + t * 32) >> 3) + 2 * (g & 1) + (pq >> 1);
            fa[t][r] = 512u * row + 16u * ((unsigned)cha ^ swz) + 8u * (pq & 1);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int chb = ((wn * 64 + t * 32) >> 3) + 2 * (g & 1) + (pq >> 1);
            fb[t][r] = 512u * row + 16u * ((unsigned)chb ^ swz) + 8u * (pq & 1);
        }
    }

#define MB_COMPUTE(buf_)                                                                                  \
    _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                                   \
        const unsigned char* st = smem + (buf_) * STAGE + ks * PIMG;                                      \
        bf16x8 af[4][NT], bf[2][NT];                                                                      \
        _Pragma("unroll") for (int pl = 0; pl < NT; ++pl) {                                               \
            _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                 \
                af[t][pl] = tr_frag(st + pl * KS * PIMG, fa[t][0], fa[t][1]);                             \
            _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                 \
                bf[t][pl] = tr_frag(st + (NT + pl) * KS * PIMG, fb[t][0], fb[t][1]);                      \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < 2; ++j) split_terms(af[i], bf[j], acc[i][j]);           \
    }
    // write-after-barrier order: at the top of stage c the registers (loaded during stage c-KS) are stored into the
    // buffer that stage c-KS just released, the loads of stage c+2KS are issued at once, then the MFMAs of stage c run
    // -> LDS always holds the current AND the next stage, the registers the one after, with ONE register set
    if (c_begin < c_end) {
        MB_LOAD(c_begin, rg0)
        MB_STORE(0, rg0)
        if (c_begin + KS < c_end) MB_LOAD(c_begin + KS, rg0)
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; c += KS) {
        const int buf = ((c - c_begin) / KS) & 1;
        if (c + KS < c_end) {
            MB_STORE(buf ^ 1, rg0)
            if (c + 2 * KS < c_end) MB_LOAD(c + 2 * KS, rg0)
        }
        MB_COMPUTE(buf)
        __syncthreads();
    }
#undef MB_COMPUTE
#undef MB_LOAD
#undef MB_STORE
#undef MB_DMA
#undef MB_DMA_ASM
#undef MB_DMA_WAIT

    float* out = p.slab + (size_t)split * p.Mi * p.Nj;
    const int col0 = tj * 256 + wn * 64 + (lane & 31);
    const int row0 = ti * 256 + wm * 128 + 4 * (lane >> 5);
    MC_STORE_TILES(4, 2)
}

template <typename K>
static int launch_big(K kernel, int smem, const MCPlanesParams& p, int wgs, hipStream_t st) {
    const int per_xcd = ceil_div(wgs, 8);
    return launch_lds(kernel, dim3(per_xcd * 8), dim3(512), smem, st, p, per_xcd);
}

// The kernels of this file behind launch_wgrad (which did the shape and extent checks):
//   MC_K_PLANES128: planes of dOut [Mk][Mi = 2C] and X [Mk][Cin] (NT planes per 32-channel chunk), 3x3 taps;
//   MC_K_PLANES256: slab[split][Mi][Nj] = A[m][Mi]^T . B[m (shifted by tap)][Cin]; taps = 9 -> Nj = 9*Cin, taps = 1 -> Nj = Cin
//                   (plain dW = dY^T . X); Mi, Cin multiples of 32;
//   MC_K_F32SRC:    plain dW straight from fp32 operands (A [Mk][lda] with Mi columns, B [Mk][ldb] with Nj columns; Mi, Nj
//                   multiples of 8), 128 x 128 tiles; colsum (optional): [splits][Mi].
// The 16x16x32 forms (default; PA2D_MC_MFMA=32 goes back) store accumulator quads with 16-byte stores: they need an aligned slab.
int launch_wgrad_planes(const MCDesc& d, const MCChoice& c, unsigned a_bytes, unsigned b_bytes, float* slab, hipStream_t st) {
    const int NT = d.engine == 2 ? 1 : 3;
    const bool mf16 = NT == 3 && pa2d_env().mc_mfma16 && (reinterpret_cast<uintptr_t>(slab) & 15) == 0;
    MCPlanesParams p = {};
    p.PA = d.A; p.PB = d.B; p.slab = slab; p.a_bytes = a_bytes; p.b_bytes = b_bytes;
    p.Mi = d.Mi; p.Nj = d.Nj; p.Mk = d.Mk; p.chunks_per_split = c.pl.chunks_per_split; p.splits = c.pl.splits;
    p.H = d.H; p.W = d.W; p.Cin = d.Cin; p.taps = d.taps;
    if (c.kernel == MC_K_PLANES256) {
        p.chA = d.Mi / 32; p.chB = d.Cin / 32;
        const int wgs = ceil_div(p.Mi, 256) * ceil_div(p.Nj, 256) * c.pl.splits;
        int rc;
        const int dma = mf16 ? (pa2d_env().mc_dma ? (pa2d_env().mc_chain ? 2 : 1) : 0) : 0;
        if (dma == 2) rc = launch_big(&gemm_mc_planes_big_kernel<3, 1, true, true, true>, 3 * 2 * 3 * 1 * 8192, p, wgs, st);
        else if (dma == 1) rc = launch_big(&gemm_mc_planes_big_kernel<3, 1, true, true>, 3 * 2 * 3 * 1 * 8192, p, wgs, st);
        else if (mf16) rc = launch_big(&gemm_mc_planes_big_kernel<3, 1, true>, 3 * 2 * 3 * 1 * 8192, p, wgs, st);      // three 16-row slots
        else if (NT == 3) rc = launch_big(&gemm_mc_planes_big_kernel<3, 1>, 2 * 2 * 3 * 1 * 8192, p, wgs, st);
        else rc = launch_big(&gemm_mc_planes_big_kernel<1, 4>, 2 * 2 * 1 * 4 * 8192, p, wgs, st);      // four 16-row K-steps per stage
        return rc;
    }
    if (!c.pl.big) return PA2D_ERR_UNSUPPORTED;
    const dim3 grid(ceil_div(d.Mi, 128) * ceil_div(d.Nj, 128) * c.pl.splits);
    if (c.kernel == MC_K_PLANES128) {
        if ((d.Mi % 128) || (d.Cin % 128) || d.taps != 9) return PA2D_ERR_UNSUPPORTED;
        p.chA = d.Mi / 32; p.chB = d.Cin / 32;
        if (NT == 3) hipLaunchKernelGGL((gemm_mc_planes_kernel<3, 1>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((gemm_mc_planes_kernel<1, 4>), grid, dim3(256), 0, st, p);
    } else {
        // F32SRC.  The three LDS slots of the 16x16x32 form allow two workgroups per CU where the 32x32x16 form runs three and
        // the kernel alone is ~10 % slower, but the step is faster with it (the chip is power-limited and the
        // kernels that follow hold a higher clock)
        p.lda = d.lda; p.ldb = d.ldb; p.colsum = d.colsum;
        if (mf16 && (d.Nj % 4) == 0) hipLaunchKernelGGL((gemm_mc_planes_kernel<3, 1, true, true>), grid, dim3(256), 0, st, p);
        else if (NT == 3) hipLaunchKernelGGL((gemm_mc_planes_kernel<3, 1, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((gemm_mc_planes_kernel<1, 4, true>), grid, dim3(256), 0, st, p);
    }
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}
