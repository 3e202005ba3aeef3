// The neural likelihood's error model (gfx950): a small MLP on (Iobs, SigIobs) per observation, differentiated every step.
//
// replaces NeuralLikelihood.call / NeuralNormalLikelihood (careless/models/likelihoods/mono.py:75-110) and tape.gradient through its network
// (careless/models/merging/variational.py:197-202):
//     delta_i = softplus(head(LeakyReLU(Dense ... (iobs_i, sigiobs_i))))        sigpred_i = sigiobs_i delta_i / mean_k(delta_k)
// The Normal log-probability itself stays where it is: the data-term kernels read sigpred in place of sigiobs (the caller swaps the
// pointer) and write ipred; from ipred this unit forms dL/dsigpred, carries it through the mean -- which couples all rows -- and through
// the network.
//
//   cl_nlik_forward : delta_kernel    lane = row, the network on the vector ALU with its weights broadcast from LDS; delta -> workspace,
//                                     one fp64 partial sum per workgroup
//                     sigpred_kernel  every workgroup adds the partial sums up in index order (the same sum, bit for bit, in all of
//                                     them), then sigpred = sigiobs delta / m in the caller's order and, with `pos`, into the layout's image
//   cl_nlik_backward: g_kernel        g_i = w_ll sum_s [1 / sigma_i - (ipred_is - iobs_i)^2 / sigma_i^3], partial sums of T = sum g_i sigma_i (fp64)
//                     wgrad_kernel    recomputes the activations, dL/ddelta_k = (g_k sigiobs_k - T / N) / m, dL/dz_k = dL/ddelta_k sigmoid(z_k),
//                                     back through the layers on the vector ALU; the weight gradient of a layer is the outer product
//                                     dZ^T A summed over rows: staged through LDS feature-major (row pitch 68 floats: the 16 feature lanes
//                                     of a ds_read_b128 fall on distinct banks) and contracted on v_mfma_f32_16x16x4_f32, 64 rows of a
//                                     wave per 16 instructions and 16 x 16 block (the map of elbo_peel.hip's peel_wgrad_kernel); bias
//                                     gradients are sums of the staged dZ.  Accumulators stay in registers for the whole launch; a
//                                     workgroup leaves ONE partial row [P_lik]; cl_reduce_partials' kernel adds the rows in index order.
// No float atomics: every sum has a fixed order, so two launches on the same inputs agree bit for bit.  Compiled WITH NaNs honoured
// (build.py): a NaN in iobs / sigiobs reaches the mean, every sigpred and every gradient entry (the non-finite stop is taken on the norm).
// fp32 arithmetic and accumulation (the reference's), the two global sums in fp64.
#include <hip/hip_runtime.h>
#include "cl_kernels.h"

namespace {

constexpr int NLIK_T = 256;                 // threads of a workgroup
constexpr int NLIK_MAX_GRID = 1024;         // workgroups of a launch = rows of the partial buffers
constexpr int NLIK_PITCH = 68;              // floats between two features of a wave's staged 64 rows
constexpr int NLIK_LMAX = 4, NLIK_WMAX = 32;

// The network's weights in LDS, zero-padded to the instance's width W (a multiple of 4): layer 0 as [x0 row | x1 row | bias]; every hidden
// layer as (in, out) [W][W] for the forward pass, its bias, and (out, in) [W][W] for the data gradient; the head's row and bias.
template <int W, int L>
struct NlikLds {
    static constexpr int HID = 3 * W;
    static constexpr int HSTRIDE = 2 * W * W + W;
    static constexpr int HEAD = HID + (L - 1) * HSTRIDE;
    static constexpr int TOTAL = HEAD + W + 4;
    static constexpr int STAGE = 2 * W * NLIK_PITCH;        // per wave: dZ [W][pitch], then the layer's input [W][pitch]
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ float nlik_act(float z, float leak) { return z > 0.0f ? z : leak * z; }
__device__ __forceinline__ float nlik_softplus(float z) { return z > 0.0f ? z + log1pf(expf(-z)) : log1pf(expf(z)); }
__device__ __forceinline__ float nlik_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

template <int W, int L>
__device__ __forceinline__ void nlik_load_weights(float* __restrict__ sw, const float* __restrict__ net, int w) {
    using X = NlikLds<W, L>;
    const int tid = threadIdx.x;
    for (int e = tid; e < X::TOTAL; e += NLIK_T) sw[e] = 0.0f;
    __syncthreads();
    for (int e = tid; e < w; e += NLIK_T) {
        sw[e] = net[2 * e];
        sw[W + e] = net[2 * e + 1];
        sw[2 * W + e] = net[2 * w + e];
    }
    int off = 3 * w;
    for (int l = 1; l < L; ++l) {
        float* b = sw + X::HID + (l - 1) * X::HSTRIDE;
        for (int e = tid; e < w * w; e += NLIK_T) {
            const int j = e / w, i = e - j * w;             // net: [out j][in i]
            const float v = net[off + e];
            b[i * W + j] = v;
            b[W * W + W + j * W + i] = v;
        }
        for (int e = tid; e < w; e += NLIK_T) b[W * W + e] = net[off + w * w + e];
        off += w * w + w;
    }
    for (int e = tid; e < w; e += NLIK_T) sw[X::HEAD + e] = net[off + e];
    if (tid == 0) sw[X::HEAD + W] = net[off + w];
    __syncthreads();
}

// the network of one row: hidden activations into h, the head's pre-activation back.  fp32 FMA chains, inputs ascending, bias first.
template <int W, int L>
__device__ __forceinline__ float nlik_net(const float* __restrict__ sw, float x0, float x1, float leak, float (&h)[L][W]) {
    using X = NlikLds<W, L>;
    // (the weights are read again for every row: hoisted out of the row loop they would take the instance's whole register file)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int g = 0; g < W / 4; ++g) {
        const f32x4 a = ld4(sw + 4 * g), b = ld4(sw + W + 4 * g), c = ld4(sw + 2 * W + 4 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) h[0][4 * g + t] = nlik_act(fmaf(b[t], x1, fmaf(a[t], x0, c[t])), leak);
    }
#pragma unroll
    for (int l = 1; l < L; ++l) {
        const float* b = sw + X::HID + (l - 1) * X::HSTRIDE;
        f32x4 acc[W / 4];
#pragma unroll
        for (int g = 0; g < W / 4; ++g) acc[g] = ld4(b + W * W + 4 * g);
#pragma unroll
        for (int i = 0; i < W; ++i) {
#pragma unroll
            for (int g = 0; g < W / 4; ++g) {
                const f32x4 wv = ld4(b + i * W + 4 * g);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[g][t] = fmaf(wv[t], h[l - 1][i], acc[g][t]);
            }
        }
#pragma unroll
        for (int g = 0; g < W / 4; ++g)
#pragma unroll
            for (int t = 0; t < 4; ++t) h[l][4 * g + t] = nlik_act(acc[g][t], leak);
    }
    float z = sw[X::HEAD + W];
#pragma unroll
    for (int g = 0; g < W / 4; ++g) {
        const f32x4 wv = ld4(sw + X::HEAD + 4 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) z = fmaf(wv[t], h[L - 1][4 * g + t], z);
    }
    return z;
}

// sum of p[0 .. n) in a fixed order, the same in every workgroup and every launch, left in all threads (sh: 4 doubles of LDS)
__device__ __forceinline__ double nlik_block_sum(const double* __restrict__ p, int n, double* sh) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += NLIK_T) s += p[k];
    s = wave_sum_d(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// a workgroup's own sum of one double per thread -> part[blockIdx.x]
__device__ __forceinline__ void nlik_block_store(double v, double* sh, double* __restrict__ part) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <int W, int L>
__global__ __launch_bounds__(NLIK_T) void nlik_delta_kernel(const float* __restrict__ iobs, const float* __restrict__ sig, const float* __restrict__ net,
                                                            int w, float leak, long long n, float* __restrict__ delta, double* __restrict__ dpart,
                                                            const int* __restrict__ stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double sh[4];
    nlik_load_weights<W, L>(lds, net, w);
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * NLIK_T + threadIdx.x; i < n; i += (long long)gridDim.x * NLIK_T) {
        float h[L][W];
        const float z = nlik_net<W, L>(lds, iobs[i], sig[i], leak, h);
        const float d = nlik_softplus(z);
        delta[i] = d;
        acc += (double)d;
    }
    nlik_block_store(acc, sh, dpart);
}

__global__ __launch_bounds__(NLIK_T) void nlik_sigpred_kernel(const float* __restrict__ sig, const float* __restrict__ delta, const double* __restrict__ dpart,
                                                              int nparts, long long n, float* __restrict__ sigpred, const int* __restrict__ pos,
                                                              float* __restrict__ sig_image, const int* __restrict__ stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    __shared__ double sh[4];
    const float m = (float)(nlik_block_sum(dpart, nparts, sh) / (double)n);
    for (long long i = (long long)blockIdx.x * NLIK_T + threadIdx.x; i < n; i += (long long)gridDim.x * NLIK_T) {
        const float sp = sig[i] * delta[i] / m;
        sigpred[i] = sp;
        if (pos != nullptr) sig_image[pos[i]] = sp;
    }
}

__global__ __launch_bounds__(NLIK_T) void nlik_g_kernel(const float* __restrict__ iobs, const float* __restrict__ sigpred, const float* __restrict__ ipred,
                                                        int S, float w_ll, long long n, float* __restrict__ g, double* __restrict__ tpart,
                                                        const int* __restrict__ stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    __shared__ double sh[4];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * NLIK_T + threadIdx.x; i < n; i += (long long)gridDim.x * NLIK_T) {
        const float io = iobs[i], sp = sigpred[i];
        const float inv = 1.0f / sp, inv3 = inv * inv * inv;
        const float* __restrict__ ip = ipred + (size_t)i * S;
        float s = 0.0f;
        for (int k = 0; k < S; ++k) {
            const float r = ip[k] - io;
            s += inv - r * r * inv3;
        }
        const float gi = w_ll * s;
        g[i] = gi;
        acc += (double)gi * (double)sp;
    }
    nlik_block_store(acc, sh, tpart);
}

// acc[ob][ib] += (dZ block ob)^T (input block ib) over the wave's 64 staged rows; bacc[ob] += this lane's share of sum_rows dZ
template <int FO, int FI, int NBO, int NBI>
__device__ __forceinline__ void nlik_outer(const float* __restrict__ Tdz, const float* __restrict__ Ta, f32x4 (&acc)[NBO][NBI], float (&bacc)[NBO],
                                           int j, int q) {
    const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 av[NBO][4], bv[NBI][4];
#pragma unroll
    for (int ob = 0; ob < NBO; ++ob) {
        const int f = 16 * ob + j;
#pragma unroll
        for (int s = 0; s < 4; ++s) av[ob][s] = f < FO ? ld4(Tdz + f * NLIK_PITCH + 16 * s + 4 * q) : zero;
    }
#pragma unroll
    for (int ib = 0; ib < NBI; ++ib) {
        const int f = 16 * ib + j;
#pragma unroll
        for (int s = 0; s < 4; ++s) bv[ib][s] = f < FI ? ld4(Ta + f * NLIK_PITCH + 16 * s + 4 * q) : zero;
    }
#pragma unroll
    for (int ob = 0; ob < NBO; ++ob) {
        float sb = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; ++s) sb += (av[ob][s][0] + av[ob][s][1]) + (av[ob][s][2] + av[ob][s][3]);
        bacc[ob] += sb;
#pragma unroll
        for (int ib = 0; ib < NBI; ++ib)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ob][ib] = mfma4(av[ob][s][t], bv[ib][s][t], acc[ob][ib]);
    }
}

// the four waves' blocks of one layer, added in wave order, into the workgroup's partial row: kernel [fo][fi] at pw, bias [fo] at pb.
// C layout of the MFMA: lane (j, q), element t = D[out 4 q + t][in j].  red: 1024 + 256 floats of LDS.
template <int NBO, int NBI>
__device__ __forceinline__ void nlik_emit(f32x4 (&acc)[NBO][NBI], float (&bacc)[NBO], float* __restrict__ red, float* __restrict__ pw,
                                          float* __restrict__ pb, int fo, int fi) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int ob = 0; ob < NBO; ++ob) {
#pragma unroll
        for (int ib = 0; ib < NBI; ++ib) {
            __syncthreads();
            *reinterpret_cast<f32x4*>(red + 4 * tid) = acc[ob][ib];
            __syncthreads();
            const int l = tid >> 2, t = tid & 3;
            const int o = 16 * ob + 4 * (l >> 4) + t, i = 16 * ib + (l & 15);
            if (o < fo && i < fi) pw[o * fi + i] = ((red[4 * l + t] + red[256 + 4 * l + t]) + red[512 + 4 * l + t]) + red[768 + 4 * l + t];
        }
        __syncthreads();
        red[1024 + tid] = bacc[ob];
        __syncthreads();
        if (tid < 16 && 16 * ob + tid < fo) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += red[1024 + 16 * k + tid];         // (wave, q) pairs in order
            pb[16 * ob + tid] = s;
        }
    }
}

template <int W, int L>
__global__ __launch_bounds__(NLIK_T) void nlik_wgrad_kernel(const float* __restrict__ iobs, const float* __restrict__ sig, const float* __restrict__ net,
                                                            int w, float leak, long long n, const float* __restrict__ g,
                                                            const double* __restrict__ dpart, const double* __restrict__ tpart, int nparts,
                                                            float* __restrict__ wpart, int P, const int* __restrict__ stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    using X = NlikLds<W, L>;
    constexpr int NB = (W + 15) / 16, LH = L > 1 ? L - 1 : 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 15, q = lane >> 4;
    float* __restrict__ Tdz = lds + X::TOTAL + wv * X::STAGE;
    float* __restrict__ Ta = Tdz + W * NLIK_PITCH;
    nlik_load_weights<W, L>(lds, net, w);
    const float m = (float)(nlik_block_sum(dpart, nparts, sh) / (double)n);
    const float tn = (float)(nlik_block_sum(tpart, nparts, sh) / (double)n);

    const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 acc0[NB][1], accH[LH][NB][NB], accO[1][NB];
    float b0[NB], bH[LH][NB], bO[1] = {0.0f};
#pragma unroll
    for (int a = 0; a < NB; ++a) {
        acc0[a][0] = zero; accO[0][a] = zero; b0[a] = 0.0f;
#pragma unroll
        for (int l = 0; l < LH; ++l) {
            bH[l][a] = 0.0f;
#pragma unroll
            for (int b = 0; b < NB; ++b) accH[l][a][b] = zero;
        }
    }

    const long long ntile = (n + 63) / 64, stride = (long long)gridDim.x * 4;
    const long long niter = (ntile + stride - 1) / stride;          // the same for every wave of the launch: the barriers below are uniform
    for (long long it = 0; it < niter; ++it) {
        const long long row = (it * stride + (long long)blockIdx.x * 4 + wv) * 64 + lane;
        const bool valid = row < n;
        const float x0 = valid ? iobs[row] : 0.0f, x1 = valid ? sig[row] : 0.0f, gk = valid ? g[row] : 0.0f;
        float h[L][W];
        const float zh = nlik_net<W, L>(lds, x0, x1, leak, h);
        const float dd = valid ? (gk * x1 - tn) / m : 0.0f;
        const float dzh = valid ? dd * nlik_sigmoid(zh) : 0.0f;
        // the head: one output, W inputs
        Tdz[lane] = dzh;
#pragma unroll
        for (int i = 0; i < W; ++i) Ta[i * NLIK_PITCH + lane] = h[L - 1][i];
        __syncthreads();
        nlik_outer<1, W, 1, NB>(Tdz, Ta, accO, bO, j, q);
        __syncthreads();
        float dh[W];
#pragma unroll
        for (int g4 = 0; g4 < W / 4; ++g4) {
            const f32x4 wh = ld4(lds + X::HEAD + 4 * g4);
#pragma unroll
            for (int t = 0; t < 4; ++t) dh[4 * g4 + t] = wh[t] * dzh;
        }
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
            float dz[W];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                dz[k] = h[l][k] > 0.0f ? dh[k] : leak * dh[k];
                Tdz[k * NLIK_PITCH + lane] = dz[k];
            }
            if (l > 0) {
#pragma unroll
                for (int i = 0; i < W; ++i) Ta[i * NLIK_PITCH + lane] = h[l - 1][i];
            } else {
                Ta[lane] = x0;
                Ta[NLIK_PITCH + lane] = x1;
            }
            __syncthreads();
            if (l > 0) nlik_outer<W, W, NB, NB>(Tdz, Ta, accH[l > 0 ? l - 1 : 0], bH[l > 0 ? l - 1 : 0], j, q);
            else nlik_outer<W, 2, NB, 1>(Tdz, Ta, acc0, b0, j, q);
            __syncthreads();
            if (l > 0) {
                const float* wb = lds + X::HID + (l - 1) * X::HSTRIDE + W * W + W;        // (out, in)
                f32x4 nd[W / 4];
#pragma unroll
                for (int g4 = 0; g4 < W / 4; ++g4) nd[g4] = zero;
#pragma unroll
                for (int k = 0; k < W; ++k) {
#pragma unroll
                    for (int g4 = 0; g4 < W / 4; ++g4) {
                        const f32x4 wvv = ld4(wb + k * W + 4 * g4);
#pragma unroll
                        for (int t = 0; t < 4; ++t) nd[g4][t] = fmaf(wvv[t], dz[k], nd[g4][t]);
                    }
                }
#pragma unroll
                for (int g4 = 0; g4 < W / 4; ++g4)
#pragma unroll
                    for (int t = 0; t < 4; ++t) dh[4 * g4 + t] = nd[g4][t];
            }
        }
    }

    // one partial row per workgroup, in the flat W^T layout on two columns
    float* __restrict__ part = wpart + (size_t)blockIdx.x * P;
    float* __restrict__ red = lds + X::TOTAL;
    nlik_emit<NB, 1>(acc0, b0, red, part, part + 2 * w, w, 2);
    int off = 3 * w;
#pragma unroll
    for (int l = 1; l < L; ++l) {
        nlik_emit<NB, NB>(accH[l - 1], bH[l - 1], red, part + off, part + off + w * w, w, w);
        off += w * w + w;
    }
    nlik_emit<1, NB>(accO, bO, red, part + off, part + off + w, 1, w);
}

inline int nlik_grid(long long n) {
    const long long g = (n + NLIK_T - 1) / NLIK_T;
    return (int)(g < 1 ? 1 : (g > NLIK_MAX_GRID ? NLIK_MAX_GRID : g));
}

inline int nlik_P(int L, int w) { return 3 * w + (L - 1) * (w * w + w) + w + 1; }

// the workspace, carved in one place: delta [n] | g [n] | (16-byte boundary) sum partials [grid] | T partials [grid] (doubles) | gradient partials [grid][P]
struct NlikWs {
    float *delta, *g, *wpart;
    double *dpart, *tpart;
    size_t bytes;
};
inline NlikWs nlik_carve(void* base, long long n, int L, int w) {
    const int G = nlik_grid(n);
    const size_t rows = ((size_t)n + 3) / 4 * 4;
    char* p = static_cast<char*>(base);
    NlikWs o;
    o.delta = reinterpret_cast<float*>(p);
    o.g = reinterpret_cast<float*>(p + 4 * rows);
    o.dpart = reinterpret_cast<double*>(p + 8 * rows);
    o.tpart = o.dpart + G;
    o.wpart = reinterpret_cast<float*>(p + 8 * rows + 16 * (size_t)G);
    o.bytes = 8 * rows + 16 * (size_t)G + 4 * (size_t)G * nlik_P(L, w);
    return o;
}

template <int W, int L>
int nlik_launch_delta(const cl_nlik_args& a, const NlikWs& ws, int G, hipStream_t st) {
    using X = NlikLds<W, L>;
    return cl_launch_lds<nlik_delta_kernel<W, L>>(dim3(G), dim3(NLIK_T), X::TOTAL * sizeof(float), st, a.iobs, a.sigiobs, a.net, a.w, a.leak, a.n, ws.delta,
                                                  ws.dpart, a.stop_flag);
}

template <int W, int L>
int nlik_launch_wgrad(const cl_nlik_args& a, const NlikWs& ws, int G, hipStream_t st) {
    using X = NlikLds<W, L>;
    return cl_launch_lds<nlik_wgrad_kernel<W, L>>(dim3(G), dim3(NLIK_T), (X::TOTAL + 4 * X::STAGE) * sizeof(float), st, a.iobs, a.sigiobs, a.net, a.w, a.leak,
                                                  a.n, (const float*)ws.g, (const double*)ws.dpart, (const double*)ws.tpart, G, ws.wpart, nlik_P(a.L, a.w),
                                                  a.stop_flag);
}

#define NLIK_BY_L(FN, WW)                              \
    switch (a.L) {                                     \
        case 1: return FN<WW, 1>(a, ws, G, st);        \
        case 2: return FN<WW, 2>(a, ws, G, st);        \
        case 3: return FN<WW, 3>(a, ws, G, st);        \
        default: return FN<WW, 4>(a, ws, G, st);       \
    }
#define NLIK_DISPATCH(FN)                              \
    if (a.w <= 4) { NLIK_BY_L(FN, 4) }                 \
    else if (a.w <= 8) { NLIK_BY_L(FN, 8) }            \
    else if (a.w <= 16) { NLIK_BY_L(FN, 16) }          \
    else { NLIK_BY_L(FN, 32) }

int nlik_delta(const cl_nlik_args& a, const NlikWs& ws, int G, hipStream_t st) { NLIK_DISPATCH(nlik_launch_delta) }
int nlik_wgrad(const cl_nlik_args& a, const NlikWs& ws, int G, hipStream_t st) { NLIK_DISPATCH(nlik_launch_wgrad) }

// what both entry points ask: -1 a missing / misaligned buffer or an empty set, -2 a network the instances do not hold
int nlik_check(const cl_nlik_args* a) {
    if (a == nullptr || a->iobs == nullptr || a->sigiobs == nullptr || a->net == nullptr || a->sigpred == nullptr || a->workspace == nullptr) return -1;
    if (a->n < 1 || (reinterpret_cast<uintptr_t>(a->workspace) & 15) != 0) return -1;
    if ((a->pos != nullptr) != (a->sig_image != nullptr)) return -1;
    if (!cl_nlik_supports(a->L, a->w)) return -2;
    return 0;
}

}  // namespace

extern "C" {

int cl_nlik_supports(int L, int w) { return L >= 1 && L <= NLIK_LMAX && w >= 1 && w <= NLIK_WMAX; }
size_t cl_nlik_param_count(int L, int w) { return (L < 1 || w < 1) ? 0 : (size_t)3 * w + (size_t)(L - 1) * ((size_t)w * w + w) + w + 1; }
int cl_nlik_grid(long long n) { return n < 1 ? 0 : nlik_grid(n); }
size_t cl_nlik_workspace_bytes(long long n, int L, int w) { return (n < 1 || !cl_nlik_supports(L, w)) ? 0 : nlik_carve(nullptr, n, L, w).bytes; }

int cl_nlik_forward(const cl_nlik_args* a, void* stream) {
    if (int e = nlik_check(a)) return e;
    hipStream_t st = (hipStream_t)stream;
    const NlikWs ws = nlik_carve(a->workspace, a->n, a->L, a->w);
    const int G = nlik_grid(a->n);
    if (int e = nlik_delta(*a, ws, G, st)) return e;
    return cl_launch<nlik_sigpred_kernel>(dim3(G), dim3(NLIK_T), st, a->sigiobs, ws.delta, ws.dpart, G, a->n, a->sigpred, a->pos, a->sig_image, a->stop_flag);
}

int cl_nlik_backward(const cl_nlik_args* a, void* stream) {
    if (int e = nlik_check(a)) return e;
    if (a->ipred == nullptr || a->d_net == nullptr || a->S < 1) return -1;
    hipStream_t st = (hipStream_t)stream;
    const NlikWs ws = nlik_carve(a->workspace, a->n, a->L, a->w);
    const int G = nlik_grid(a->n);
    if (int e = cl_launch<nlik_g_kernel>(dim3(G), dim3(NLIK_T), st, a->iobs, a->sigpred, a->ipred, a->S, a->w_ll, a->n, ws.g, ws.tpart, a->stop_flag)) return e;
    if (int e = nlik_wgrad(*a, ws, G, st)) return e;
    return cl_launch_reduce_partials(ws.wpart, G, nlik_P(a->L, a->w), a->d_net, a->stop_flag, st);       // index order: deterministic
}

}  // extern "C"
