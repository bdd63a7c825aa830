// Head attention of the merged SequenSolver (reference SequenSolverMerged.py, SequenSolver.attention): the [T, dim]
// LayerNorm output of a sample, read as contiguous memory, is cut into `heads` groups of T pseudo-rows of sd = dim / heads
// floats; every group gets the same three bias-free Linear(sd, sd) and a (causal) softmax attention among its T rows.
//
//   q, k, v = x Wq^T, x Wk^T, x Wv^T      [T, sd]       attn = softmax_T(q k^T * scale, entries j > i masked)     [T, T]
//   out = attn v (+ res)                  [T, sd]
//
// With T <= 32 and sd <= 64 a group is at most 8 KiB and the three weight matrices at most 48 KiB: everything fits one
// workgroup's LDS, so projections, scores, softmax and the product with v are ONE launch (the unfused route is three GEMM
// launches of [G*T, sd] x [sd, sd] plus the two of pa2d_seq_attn).  A workgroup stages the weights once and then walks
// its fixed set of groups g = blockIdx.x, blockIdx.x + gridDim.x, ...; gridDim.x = min(G, NWG_MAX).
//
// The forward saves attn [G, T, T] only; the backward recomputes q, k, v from x with the forward's code (same bits).
//   dA = dout v^T (fp64 sums)      ds = attn * sum_k attn_k (dA_j - dA_k) * scale      (cancellation-free form)
//   dq = ds k, dk = ds^T q, dv = attn^T dout        dx = dq Wq + dk Wk + dv Wv         (plain store)
//   dWq = dq^T x, dWk = dk^T x, dWv = dv^T x        summed in registers over the workgroup's groups, one record per
//                                                   workgroup; a second launch adds the <= NWG_MAX records in fp64.
// fp32 FMA on the VALU (fp64 for the projection and score sums) on every engine; every sum runs in a fixed order inside
// one thread, so results repeat bit for bit.  No allocation, no static state, no atomics.
#include "pa2d_internal.h"

namespace {

constexpr int NT = 256;
constexpr int TMAX = 32;         // rows of a group
constexpr int SD_MAX = 64;       // width of a group
constexpr int NWG_MAX = 32;      // workgroups of a launch = partial records of the weight gradients
constexpr int SP = TMAX + 1;     // pitch of a [T, T] matrix in LDS

// LDS layout (floats).  Rows of the weights and of the [T, sd] tiles have pitch P = sd + 4: 16-byte aligned, and row r
// starts 4 r banks further (mod 64), so float4 reads of one column block by consecutive rows do not collide.
__host__ __device__ inline int pitch_of(int sd) { return sd + 4; }
inline size_t lds_bytes(int T, int sd, int tiles, int mats) {
    const size_t P = (size_t)pitch_of(sd);
    return sizeof(float) * (3 * sd * P + (size_t)tiles * T * P + (size_t)mats * T * SP);
}
constexpr int FWD_TILES = 4, FWD_MATS = 1;      // x, q, k, v; attn
constexpr int BWD_TILES = 7, BWD_MATS = 3;      // x, dout, q, k, v (then dv), dq, dk; attn, dA, ds

__device__ __forceinline__ void stage_rows(float* dst, const float* __restrict__ src, int rows, int sd, int P, int tid) {
    const int q4 = sd >> 2;
    for (int e = tid; e < rows * q4; e += NT) {
        const int r = e / q4, c = (e % q4) << 2;
        *reinterpret_cast<float4*>(dst + r * P + c) = *reinterpret_cast<const float4*>(src + (long long)r * sd + c);
    }
}

// q, k, v [T, sd] = x W^T for the three staged weight matrices (row o of W against row t of x).  The sums run in fp64,
// where a product of two floats is exact, and are rounded to fp32 once: q and k feed the differences of nearly equal
// scores, and 3 T sd^2 fp64 FMAs (31 k per group at the reference's shape) cost nothing beside a launch
__device__ __forceinline__ void project(const float* xs, const float* w, float* qs, float* ks, float* vs, int T, int sd,
                                        int P, int tid) {
    const int q4 = sd >> 2;
    for (int e = tid; e < T * sd; e += NT) {
        const int t = e / sd, o = e % sd;
        const float4* xr = reinterpret_cast<const float4*>(xs + t * P);
        const float4* a = reinterpret_cast<const float4*>(w + o * P);
        const float4* b = reinterpret_cast<const float4*>(w + (sd + o) * P);
        const float4* c = reinterpret_cast<const float4*>(w + (2 * sd + o) * P);
        double q0 = 0.0, q1 = 0.0, k0 = 0.0, k1 = 0.0, v0 = 0.0, v1 = 0.0;
        for (int i = 0; i < q4; ++i) {
            const float4 u = xr[i], wa = a[i], wb = b[i], wc = c[i];
            const double ux = u.x, uy = u.y, uz = u.z, uw = u.w;
            q0 = fma(ux, (double)wa.x, q0); q1 = fma(uy, (double)wa.y, q1); q0 = fma(uz, (double)wa.z, q0); q1 = fma(uw, (double)wa.w, q1);
            k0 = fma(ux, (double)wb.x, k0); k1 = fma(uy, (double)wb.y, k1); k0 = fma(uz, (double)wb.z, k0); k1 = fma(uw, (double)wb.w, k1);
            v0 = fma(ux, (double)wc.x, v0); v1 = fma(uy, (double)wc.y, v1); v0 = fma(uz, (double)wc.z, v0); v1 = fma(uw, (double)wc.w, v1);
        }
        qs[t * P + o] = (float)(q0 + q1);
        ks[t * P + o] = (float)(k0 + k1);
        vs[t * P + o] = (float)(v0 + v1);
    }
}

// m[i][j] = <a_i, b_j> over sd channels, summed in fp64 (products of floats are exact there); masked entries are 0
__device__ __forceinline__ void scores(const float* as, const float* bs, float* m, int T, int sd, int P, int causal, int tid) {
    const int q4 = sd >> 2;
    for (int e = tid; e < T * T; e += NT) {
        const int i = e / T, j = e % T;
        double a0 = 0.0, a1 = 0.0;
        if (!causal || j <= i) {
            const float4* ar = reinterpret_cast<const float4*>(as + i * P);
            const float4* br = reinterpret_cast<const float4*>(bs + j * P);
            for (int c = 0; c < q4; ++c) {
                const float4 u = ar[c], w = br[c];
                a0 = fma((double)u.x, (double)w.x, a0);
                a1 = fma((double)u.y, (double)w.y, a1);
                a0 = fma((double)u.z, (double)w.z, a0);
                a1 = fma((double)u.w, (double)w.w, a1);
            }
        }
        m[i * SP + j] = (float)(a0 + a1);
    }
}

__device__ __forceinline__ void fma4(float4& a, float w, const float4 v) {
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
}

__global__ __launch_bounds__(NT) void head_attn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                           const float* __restrict__ wk, const float* __restrict__ wv,
                                                           const float* __restrict__ res, float* __restrict__ out,
                                                           float* __restrict__ attn, int G, int T, int sd, float scale,
                                                           int causal) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, P = pitch_of(sd), q4 = sd >> 2;
    float* w = lds;
    float* xs = w + 3 * sd * P;
    float* qs = xs + T * P;
    float* ks = qs + T * P;
    float* vs = ks + T * P;
    float* al = vs + T * P;
    stage_rows(w, wq, sd, sd, P, tid);
    stage_rows(w + sd * P, wk, sd, sd, P, tid);
    stage_rows(w + 2 * sd * P, wv, sd, sd, P, tid);
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const long long base = (long long)g * T * sd;
        __syncthreads();                               // the previous group's readers are done (first pass: nothing)
        stage_rows(xs, x + base, T, sd, P, tid);
        __syncthreads();
        project(xs, w, qs, ks, vs, T, sd, P, tid);
        __syncthreads();
        scores(qs, ks, al, T, sd, P, causal, tid);
        __syncthreads();
        if (tid < T) {
            float* row = al + tid * SP;
            float* o = attn + ((long long)g * T + tid) * T;
            const int n = causal ? tid + 1 : T;
            float mx = -INFINITY;
            for (int j = 0; j < n; ++j) mx = fmaxf(mx, row[j] * scale);
            float sum = 0.f;
            for (int j = 0; j < n; ++j) sum += expf(row[j] * scale - mx);
            for (int j = 0; j < n; ++j) {
                const float p = expf(row[j] * scale - mx) / sum;
                row[j] = p;
                o[j] = p;
            }
            for (int j = n; j < T; ++j) {
                row[j] = 0.f;
                o[j] = 0.f;
            }
        }
        __syncthreads();
        for (int e = tid; e < T * q4; e += NT) {
            const int t = e / q4, c = (e % q4) << 2;
            const int n = causal ? t + 1 : T;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < n; ++j) fma4(a, al[t * SP + j], *reinterpret_cast<const float4*>(vs + j * P + c));
            if (res) {
                const float4 r = *reinterpret_cast<const float4*>(res + base + (long long)t * sd + c);
                a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
            }
            *reinterpret_cast<float4*>(out + base + (long long)t * sd + c) = a;
        }
    }
}

// rec: [gridDim.x][3][sd][sd] partial weight gradients (dWq, dWk, dWv), every element written
__global__ __launch_bounds__(NT) void head_attn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                           const float* __restrict__ wk, const float* __restrict__ wv,
                                                           const float* __restrict__ attn, const float* __restrict__ dout,
                                                           float* __restrict__ dx, float* __restrict__ rec, int G, int T,
                                                           int sd, float scale, int causal) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, P = pitch_of(sd), q4 = sd >> 2;
    float* w = lds;
    float* xs = w + 3 * sd * P;
    float* dos = xs + T * P;
    float* qs = dos + T * P;
    float* ks = qs + T * P;
    float* vs = ks + T * P;              // v until dA is formed, then dv
    float* dql = vs + T * P;
    float* dkl = dql + T * P;
    float* al = dkl + T * P;
    float* dal = al + T * SP;
    float* dsl = dal + T * SP;
    stage_rows(w, wq, sd, sd, P, tid);
    stage_rows(w + sd * P, wk, sd, sd, P, tid);
    stage_rows(w + 2 * sd * P, wv, sd, sd, P, tid);
    // this thread's elements (o, c .. c+3) of the three weight gradients: e = tid + s * NT < sd * sd / 4
    float4 aq[4], ak[4], av[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) aq[s] = ak[s] = av[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const long long base = (long long)g * T * sd;
        __syncthreads();
        stage_rows(xs, x + base, T, sd, P, tid);
        stage_rows(dos, dout + base, T, sd, P, tid);
        for (int e = tid; e < T * T; e += NT) al[(e / T) * SP + e % T] = attn[(long long)g * T * T + e];
        __syncthreads();
        project(xs, w, qs, ks, vs, T, sd, P, tid);
        __syncthreads();
        scores(dos, vs, dal, T, sd, P, causal, tid);
        __syncthreads();
        if (tid < T) {
            const float* a = al + tid * SP;
            const float* d = dal + tid * SP;
            float* o = dsl + tid * SP;
            const int n = causal ? tid + 1 : T;
            // dA_j - <a, dA> written as sum_k a_k (dA_j - dA_k) (sum a = 1): nothing is lost to cancellation near one-hot rows
            for (int j = 0; j < n; ++j) {
                float s = 0.f;
                for (int k = 0; k < n; ++k) s = fmaf(a[k], d[j] - d[k], s);
                o[j] = a[j] * s * scale;
            }
            for (int j = n; j < T; ++j) o[j] = 0.f;
        }
        __syncthreads();
        for (int e = tid; e < T * q4; e += NT) {
            const int t = e / q4, c = (e % q4) << 2;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q;
            for (int j = 0; j < T; ++j) {
                fma4(q, dsl[t * SP + j], *reinterpret_cast<const float4*>(ks + j * P + c));       // dq = ds k
                fma4(k, dsl[j * SP + t], *reinterpret_cast<const float4*>(qs + j * P + c));       // dk = ds^T q
                fma4(v, al[j * SP + t], *reinterpret_cast<const float4*>(dos + j * P + c));       // dv = attn^T dout
            }
            *reinterpret_cast<float4*>(dql + t * P + c) = q;
            *reinterpret_cast<float4*>(dkl + t * P + c) = k;
            *reinterpret_cast<float4*>(vs + t * P + c) = v;      // nothing reads v in this step
        }
        __syncthreads();
        for (int e = tid; e < T * q4; e += NT) {                 // dx = dq Wq + dk Wk + dv Wv
            const int t = e / q4, c = (e % q4) << 2;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int o = 0; o < sd; ++o) fma4(a, dql[t * P + o], *reinterpret_cast<const float4*>(w + o * P + c));
            for (int o = 0; o < sd; ++o) fma4(a, dkl[t * P + o], *reinterpret_cast<const float4*>(w + (sd + o) * P + c));
            for (int o = 0; o < sd; ++o) fma4(a, vs[t * P + o], *reinterpret_cast<const float4*>(w + (2 * sd + o) * P + c));
            *reinterpret_cast<float4*>(dx + base + (long long)t * sd + c) = a;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {                            // dW[o][c] += sum_t d[t][o] x[t][c]
            const int e = tid + s * NT;
            if (e < sd * q4) {
                const int o = e / q4, c = (e % q4) << 2;
                for (int t = 0; t < T; ++t) {
                    const float4 xv = *reinterpret_cast<const float4*>(xs + t * P + c);
                    fma4(aq[s], dql[t * P + o], xv);
                    fma4(ak[s], dkl[t * P + o], xv);
                    fma4(av[s], vs[t * P + o], xv);
                }
            }
        }
    }
    const int dd = sd * sd;
    float* r = rec + (long long)blockIdx.x * 3 * dd;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = tid + s * NT;
        if (e < sd * q4) {
            *reinterpret_cast<float4*>(r + e * 4) = aq[s];
            *reinterpret_cast<float4*>(r + dd + e * 4) = ak[s];
            *reinterpret_cast<float4*>(r + 2 * dd + e * 4) = av[s];
        }
    }
}

// dwq | dwk | dwv (+)= the sum of the nrec records, record 0 first, in fp64
__global__ __launch_bounds__(NT) void head_attn_dw_kernel(const float* __restrict__ rec, int nrec, int dd,
                                                          float* __restrict__ dwq, float* __restrict__ dwk,
                                                          float* __restrict__ dwv, int accumulate) {
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= 3 * dd) return;
    double s = 0.0;
    for (int r = 0; r < nrec; ++r) s += (double)rec[(long long)r * 3 * dd + idx];
    float* d = idx < dd ? dwq + idx : idx < 2 * dd ? dwk + (idx - dd) : dwv + (idx - 2 * dd);
    *d = accumulate ? *d + (float)s : (float)s;
}

int check_shape(int G, int T, int sd) {
    if (T < 1 || T > TMAX) return PA2D_ERR_UNSUPPORTED;
    if (sd < 4 || (sd & 3) || sd > SD_MAX) return PA2D_ERR_UNSUPPORTED;
    if (G < 0) return PA2D_ERR_ARG;
    if ((unsigned long long)G * T * sd * 4ull >= 0xFFFFFFF0ull) return PA2D_ERR_UNSUPPORTED;
    return PA2D_OK;
}
bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
int nwg_of(int G) { return G < NWG_MAX ? G : NWG_MAX; }

template <typename K>
int raise_lds_limit(K kernel, size_t smem) {
    if (smem <= 64 * 1024) return PA2D_OK;
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)smem);
}

}  // namespace

extern "C" {

int pa2d_head_seq_attn_fwd(const float* x, const float* wq, const float* wk, const float* wv, const float* res, float* out,
                           float* attn, int G, int T, int sd, float scale, int causal, void* stream) {
    const int rc = check_shape(G, T, sd);
    if (rc) return rc;
    if (G == 0) return PA2D_OK;
    if (!x || !wq || !wk || !wv || !out || !attn) return PA2D_ERR_ARG;
    if (misaligned(x) || misaligned(wq) || misaligned(wk) || misaligned(wv) || misaligned(res) || misaligned(out))
        return PA2D_ERR_ARG;
    const size_t smem = lds_bytes(T, sd, FWD_TILES, FWD_MATS);
    const int ra = raise_lds_limit(&head_attn_fwd_kernel, smem);
    if (ra) return ra;
    hipLaunchKernelGGL(head_attn_fwd_kernel, dim3(nwg_of(G)), dim3(NT), smem, (hipStream_t)stream, x, wq, wk, wv, res, out,
                       attn, G, T, sd, scale, causal ? 1 : 0);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

size_t pa2d_head_seq_attn_bwd_workspace(int G, int T, int sd) {
    if (G <= 0 || check_shape(G, T, sd)) return 0;
    return sizeof(float) * (size_t)nwg_of(G) * 3 * sd * sd;
}

int pa2d_head_seq_attn_bwd(const float* x, const float* wq, const float* wk, const float* wv, const float* attn,
                           const float* dout, float* dx, float* dwq, float* dwk, float* dwv, void* ws, size_t ws_bytes,
                           int G, int T, int sd, float scale, int causal, int accumulate, void* stream) {
    const int rc = check_shape(G, T, sd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (G == 0) {
        if (accumulate) return PA2D_OK;
        const size_t wb = sizeof(float) * (size_t)sd * sd;
        int rz = pa2d_zero(dwq, wb, st);
        if (!rz) rz = pa2d_zero(dwk, wb, st);
        return rz ? rz : pa2d_zero(dwv, wb, st);
    }
    if (!x || !wq || !wk || !wv || !attn || !dout || !dx || !dwq || !dwk || !dwv) return PA2D_ERR_ARG;
    if (misaligned(x) || misaligned(wq) || misaligned(wk) || misaligned(wv) || misaligned(dout) || misaligned(dx) ||
        misaligned(ws))
        return PA2D_ERR_ARG;
    if (!ws || ws_bytes < pa2d_head_seq_attn_bwd_workspace(G, T, sd)) return PA2D_ERR_WORKSPACE;
    const size_t smem = lds_bytes(T, sd, BWD_TILES, BWD_MATS);
    const int ra = raise_lds_limit(&head_attn_bwd_kernel, smem);
    if (ra) return ra;
    const int nwg = nwg_of(G);
    hipLaunchKernelGGL(head_attn_bwd_kernel, dim3(nwg), dim3(NT), smem, st, x, wq, wk, wv, attn, dout, dx, (float*)ws, G,
                       T, sd, scale, causal ? 1 : 0);
    PA2D_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_attn_dw_kernel, dim3(ceil_div(3 * sd * sd, NT)), dim3(NT), 0, st, (const float*)ws, nwg,
                       sd * sd, dwq, dwk, dwv, accumulate);
    PA2D_CHECK_LAUNCH();
    return PA2D_OK;
}

}  // extern "C"
