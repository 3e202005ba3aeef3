// The output step (gfx950; include/careless_hip.h: "output step: merged amplitudes", "... posterior predictive moments per observation")
// and the noise diagnostic: once per run, fp64 where a subtraction cancels.  Direct tests: tests/test_output_step.py.
//
//   tn_moments_kernel        mean, standard deviation, fourth raw moment of the truncated-normal q(F)   [surrogate_posteriors.py:55-73]
//   rw_moments_kernel        the same of the Rice-Woolfson posterior                                   [surrogate_posteriors.py:156-163]
//   predict_moments_kernel   E[I], var[I] per observation                                              [variational.py:80-121]
//   noise_kernel             the numbers the step's kernels would draw for (seed, step)
#include <hip/hip_runtime.h>
#include "cl_math.h"
#include "cl_kernels.h"

// Output step (include/careless_hip.h: cl_tn_moments): mean, standard deviation and fourth raw moment of q(F_h) = Normal(loc, scale)
// truncated to [low, high], from the raw vectors; reference surrogate_posteriors.py:55-73 (_tf_moment_4: the closed form of Orjebin's
// note) and the TFP truncated-normal moments behind .mean() / .stddev().  fp64: once per run over R values, and the caller subtracts
// <F^2>^2 from <F^4>.  With alpha = (low - loc) / scale <= ~0 (loc = exp(a) > 0 >= low) the normaliser Phi(beta) - Phi(alpha) is
// taken as (erfc(alpha / sqrt 2) - erfc(beta / sqrt 2)) / 2: no cancellation on the side that matters.
__global__ __launch_bounds__(256) void tn_moments_kernel(const float* __restrict__ qa, const float* __restrict__ qb, const float* __restrict__ low, int R,
                                                         double high, double high4, float eps, float* __restrict__ mean, float* __restrict__ sd,
                                                         double* __restrict__ m4) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const double mu = (double)expf(qa[r]), sg = (double)(expf(qb[r]) + eps), a = (double)low[r];
    constexpr double RSQRT2 = 0.70710678118654752440, RSQRT2PI = 0.39894228040143267794;
    const double za = (a - mu) / sg;
    const double pa = RSQRT2PI * exp(-0.5 * za * za);
    if (mean != nullptr || sd != nullptr) {
        const bool open = !(high < 1e30);
        const double zb = open ? 0.0 : (high - mu) / sg;
        const double pb = open ? 0.0 : RSQRT2PI * exp(-0.5 * zb * zb);
        const double zn = 0.5 * (erfc(za * RSQRT2) - (open ? 0.0 : erfc(zb * RSQRT2)));
        const double ratio = (pa - pb) / zn;
        if (mean != nullptr) mean[r] = (float)(mu + sg * ratio);
        if (sd != nullptr) {
            const double bpb = pb > 0.0 ? zb * pb : 0.0;
            sd[r] = (float)sqrt(sg * sg * (1.0 + (za * pa - bpb) / zn - ratio * ratio));
        }
    }
    if (m4 != nullptr) {
        const bool open = !(high4 < 1e30);
        double bterm = 0.0, cb = 0.0;
        if (!open) {
            const double b = high4, zb = (b - mu) / sg;
            bterm = (b * b * b + b * b * mu + b * mu * mu + sg * sg * (3.0 * b + 5.0 * mu) + mu * mu * mu) * RSQRT2PI * exp(-0.5 * zb * zb);
            cb = erfc(zb * RSQRT2);
        }
        const double aterm = (a * a * a + a * a * mu + a * mu * mu + sg * sg * (3.0 * a + 5.0 * mu) + mu * mu * mu) * pa;
        const double den = 0.5 * (erfc(za * RSQRT2) - cb);
        m4[r] = mu * mu * mu * mu + 6.0 * mu * mu * sg * sg + 3.0 * sg * sg * sg * sg - sg * (bterm - aterm) / den;
    }
}

// Exponentially scaled modified Bessel functions I0(x) e^-x, I1(x) e^-x in fp64 for x >= 0: the ascending series (all terms positive) up to
// 30, Hankel's asymptotic expansion beyond (smallest term < e^-60 there); both summed until a term no longer counts.
__device__ void i0e_i1e_d(double x, double* i0e, double* i1e) {
    if (x <= 30.0) {
        const double q = 0.25 * x * x;
        double t0 = 1.0, s0 = 1.0, t1 = 0.5 * x, s1 = t1;
        for (int k = 1; k < 200; ++k) {
            t0 *= q / ((double)k * k);
            t1 *= q / ((double)k * (k + 1));
            s0 += t0; s1 += t1;
            if (t0 < 1e-17 * s0 && t1 < 1e-17 * s1) break;
        }
        const double e = exp(-x);
        *i0e = s0 * e; *i1e = s1 * e;
        return;
    }
    const double r = 1.0 / (8.0 * x);
    double t0 = 1.0, s0 = 1.0, t1 = 1.0, s1 = 1.0;
    for (int k = 1; k < 60; ++k) {
        const double m = (2.0 * k - 1.0) * (2.0 * k - 1.0);
        t0 *= -(0.0 - m) * r / k;
        t1 *= -(4.0 - m) * r / k;
        s0 += t0; s1 += t1;
        if (fabs(t0) < 1e-17 * s0 && fabs(t1) < 1e-17 * s1) break;
    }
    const double f = 1.0 / sqrt(6.283185307179586477 * x);
    *i0e = s0 * f; *i1e = s1 * f;
}

// Output step (include/careless_hip.h: cl_rw_moments): mean, standard deviation and fourth raw moment of the Rice-Woolfson posterior from
// the raw vectors, fp64 (the variance nu^2 + 2 sigma^2 - mean^2 cancels by (nu / sigma)^2).  The formulas of RiceWoolfson._moments
// (careless_amd/models/merging/surrogate_posteriors.py): no normal-limit crossover at nu / sigma > 40.
__global__ __launch_bounds__(256) void rw_moments_kernel(const float* __restrict__ qa, const float* __restrict__ qb, const unsigned char* __restrict__ centric,
                                                         int R, float eps, float* __restrict__ mean, float* __restrict__ sd, double* __restrict__ m4) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const double mu = (double)expf(qa[r]), sg = (double)(expf(qb[r]) + eps);
    const bool c = centric[r] != 0;
    const double mu2 = mu * mu, sg2 = sg * sg;
    if (mean != nullptr || sd != nullptr) {
        double m, var;
        if (c) {
            const double y = mu / sg;
            m = sg * 0.79788456080286535588 * exp(-0.5 * y * y) + mu * erf(y * 0.70710678118654752440);
            var = mu2 + sg2 - m * m;
        } else {
            const double t = 0.5 * mu2 / sg2;
            double i0e, i1e;
            i0e_i1e_d(0.5 * t, &i0e, &i1e);
            m = sg * 1.25331413731550025121 * ((1.0 + t) * i0e + t * i1e);
            var = 2.0 * sg2 + mu2 - m * m;
        }
        if (mean != nullptr) mean[r] = (float)m;
        if (sd != nullptr) sd[r] = (float)sqrt(fmax(var, 0.0));
    }
    if (m4 != nullptr) m4[r] = c ? mu2 * mu2 + 6.0 * mu2 * sg2 + 3.0 * sg2 * sg2 : mu2 * mu2 + 8.0 * sg2 * mu2 + 8.0 * sg2 * sg2;
}

// Output step, per observation (reference VariationalMergingModel.prediction_mean_stddev, careless/models/merging/variational.py:80-121): with
// the scale's moments (smean, sstd) of the row and <F^2> = mean^2 + std^2, <F^4> of its reflection, E[I] = smean <F^2> and
// var[I] = <F^4> (smean^2 + sstd^2) - E[I]^2, in fp64 (the subtraction cancels).  HBM-bound: 12 bytes in, 16 out per row + two gathers.
__global__ __launch_bounds__(256) void predict_moments_kernel(const float* __restrict__ smean, const float* __restrict__ sstd, const int* __restrict__ refl_id,
                                                              long long n, const float* __restrict__ fmean, const float* __restrict__ fstd,
                                                              const double* __restrict__ fm4, int R, double* __restrict__ iexp, double* __restrict__ ivar) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = refl_id[i];
        const bool ok = r >= 0 && r < R;
        const double m = ok ? (double)fmean[r] : 0.0, s = ok ? (double)fstd[r] : 0.0, m4 = ok ? fm4[r] : 0.0;
        const double sm = (double)smean[i], ss = (double)sstd[i];
        const double e = sm * (m * m + s * s);
        iexp[i] = e;
        ivar[i] = m4 * (sm * sm + ss * ss) - e * e;
    }
}

// debug / test aid: the noise the kernels would draw for (seed, step)
__global__ void noise_kernel(unsigned long long seed, unsigned step, int S, long long n, long long offset, int kind,
                             float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 2) {                     // the Rice-Woolfson posterior's pairs: out[n][S][2]
        for (int s = 0; s < S; ++s)
            cl_noise_rw_pick(cl_noise_rw_block(seed, step, (uint32_t)s, (uint64_t)(offset + i)), (uint32_t)s, out + 2 * ((size_t)i * S + s),
                             out + 2 * ((size_t)i * S + s) + 1);
        return;
    }
    for (int s = 0; s < S; ++s)
        out[(size_t)i * S + s] = (kind == 0) ? cl_noise_uniform(seed, step, (uint32_t)s, (uint64_t)(offset + i))
                                             : cl_noise_normal(seed, step, (uint32_t)s, (uint64_t)(offset + i));
}

extern "C" {

int cl_tn_moments(const float* q_loc_raw, const float* q_scale_raw, const float* low, int R, double high_moments, double high_m4, float eps,
                  float* mean, float* std, double* m4, void* stream) {
    if (q_loc_raw == nullptr || q_scale_raw == nullptr || low == nullptr || R < 1) return -1;
    if (mean == nullptr && std == nullptr && m4 == nullptr) return -1;
    return cl_launch<tn_moments_kernel>(dim3((unsigned)((R + 255) / 256)), dim3(256), (hipStream_t)stream, q_loc_raw, q_scale_raw, low, R, high_moments,
                                        high_m4, eps, mean, std, m4);
}

// (replaces RiceWoolfson.mean / .stddev, reference surrogate_posteriors.py:156-163; the fourth moment is this project's)
int cl_rw_moments(const float* q_loc_raw, const float* q_scale_raw, const unsigned char* q_centric, int R, float eps, float* mean, float* std,
                  double* m4, void* stream) {
    if (q_loc_raw == nullptr || q_scale_raw == nullptr || q_centric == nullptr || R < 1) return -1;
    if (mean == nullptr && std == nullptr && m4 == nullptr) return -1;
    return cl_launch<rw_moments_kernel>(dim3((unsigned)((R + 255) / 256)), dim3(256), (hipStream_t)stream, q_loc_raw, q_scale_raw, q_centric, R, eps, mean,
                                        std, m4);
}

int cl_predict_moments(const float* scale_mean, const float* scale_std, const int* refl_id, long long n, const float* f_mean, const float* f_std,
                       const double* f_m4, int R, double* iexp, double* ivar, void* stream) {
    if (scale_mean == nullptr || scale_std == nullptr || refl_id == nullptr || f_mean == nullptr || f_std == nullptr || f_m4 == nullptr ||
        iexp == nullptr || ivar == nullptr || n < 1 || R < 1)
        return -1;
    long long blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    return cl_launch<predict_moments_kernel>(dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, scale_mean, scale_std, refl_id, n, f_mean, f_std, f_m4,
                                             R, iexp, ivar);
}

int cl_debug_noise(unsigned long long seed, unsigned step, int S, long long n, long long offset, int kind, float* out,
                   void* stream) {
    if (out == nullptr || S < 1 || n < 1) return -1;
    return cl_launch<noise_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)stream, seed, step, S, n, offset, kind, out);
}

}  // extern "C"
