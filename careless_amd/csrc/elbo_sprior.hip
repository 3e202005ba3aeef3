// The KL term on the scale distribution, "Σ KLDiv" (gfx950; include/careless_hip.h: cl_scale_kl).
//
// Reference: VariationalMergingModel.call with a scale_prior (careless/models/merging/variational.py:156-163) through add_kl_div
// (:123-139) with weight 1 and reduction 'mean': kl_div = scale_dist.kl_divergence(scale_prior) where TFP has one registered (a bare
// Normal against a Normal prior: the ANALYTIC form), else scale_dist.log_prob(z_scale) - scale_prior.log_prob(z_scale) on the step's
// own samples (the SAMPLE form), z = a_i (loc_i + sigma_i eta_is + c) through tfb.Shift(c) (scaling/nn.py:84-87) and tfb.Scale(a_i)
// (scaling/image.py:60-63).
//
// The launch sits between the slot likelihood, which has filled dO = dL/d(loc, sigma) per row, and cl_mlp_backward_ext, which takes dO
// through the scaler: a regulariser on (loc, sigma) per row that touches no fused kernel.  Thread = row, loop over the samples, eta from
// the noise function the slot kernels use (cl_noise_normal on the same key: the data term's draw bit for bit).  The thread that owns the
// row adds the two derivatives into dO with a plain read-modify-write; the value leaves the kernel as one fp64 partial per workgroup,
// which a one-wave launch behind it adds up in a fixed order -- no float atomic on the value's way, two calls on the same inputs agree
// bit for bit.  Compiled with NaNs honoured (build.py): a NaN in loc or sigma reaches the value and both derivatives.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cl_math.h"
#include "cl_kernels.h"

namespace {

constexpr int SPRIOR_T = 256;

__global__ __launch_bounds__(SPRIOR_T) void scale_kl_kernel(const cl_sprior_args A, const float t_const) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * SPRIOR_T;
    const long long rounds = ((long long)A.n + stride - 1) / stride;       // every thread runs them all: the image sums are wave-wide
    const float w = A.weight, m = A.p_loc, sc = A.p_scale;
    double acc = 0.0;
    for (long long r = 0; r < rounds; ++r) {
        const long long i = r * stride + (long long)blockIdx.x * SPRIOR_T + threadIdx.x;
        const bool act = i < (long long)A.n;
        int im = 0;
        float da = 0.0f;
        if (act) {
            const float loc = A.loc[i], sigma = A.sigma[i];
            float dloc, dsig, term;
            if (A.form == CL_SPRIOR_ANALYTIC) {
                // KL(N(loc, sigma) || N(m, s)) = log(s / sigma) + (sigma^2 + (loc - m)^2) / (2 s^2) - 1/2
                const float is2 = 1.0f / (sc * sc), dm = loc - m;
                term = logf(sc / sigma) + 0.5f * (sigma * sigma + dm * dm) * is2 - 0.5f;
                dloc = dm * is2;
                dsig = sigma * is2 - 1.0f / sigma;
            } else {
                float aim = 1.0f;
                if (A.use_img) { im = A.image_id[i]; if (im > 0) aim = A.img[im - 1]; }
                const uint64_t gidx = A.row_index ? (uint64_t)A.row_index[i] : (uint64_t)(A.obs_offset + i);
                const float inv_s = 1.0f / (float)A.S;
                float lp = 0.0f, e2 = 0.0f, g = 0.0f, ge = 0.0f, gy = 0.0f;
                for (int s = 0; s < A.S; ++s) {
                    const float eta = A.eta ? A.eta[(size_t)i * A.S + s] : cl_noise_normal(A.seed, A.step, (uint32_t)s, gidx);
                    const float y = loc + sigma * eta + A.shift;
                    float dz;
                    lp += cl_ref_prior_log_prob(A.kind, aim * y, m, sc, false, A.p_df, t_const, &dz);
                    e2 += eta * eta;
                    g += dz; ge += dz * eta; gy += dz * y;
                }
                // mean over s of log q(z) - l(z), log q(z) = -log sigma - eta^2 / 2 - log(2 pi) / 2 - log|a|
                term = -logf(sigma) - 0.5f * CL_LOG_2PI_F - logf(fabsf(aim)) - (0.5f * e2 + lp) * inv_s;
                dloc = -aim * g * inv_s;
                dsig = -1.0f / sigma - aim * ge * inv_s;
                da = w * (-1.0f / aim - gy * inv_s);
            }
            acc += (double)term;
            A.dO[2 * (size_t)i] += w * dloc;
            A.dO[2 * (size_t)i + 1] += w * dsig;
        }
        if (A.form == CL_SPRIOR_SAMPLE && A.use_img) {           // (wave-uniform)
            if (A.dimg_obs != nullptr) {
                if (act && im > 0) A.dimg_obs[i] += da;          // deterministic records: summed per image, in row order, by cl_det_reduce
            } else {
                // rows are (nearly) ordered by image, so a wave usually holds one image: one wave sum, one atomic (image 0 is pinned to 1)
                const bool take = act && im > 0;
                const unsigned long long mk = __ballot(take);
                if (mk != 0ull) {
                    const int im0 = __builtin_amdgcn_readlane(im, __builtin_ctzll(mk));
                    if (__all(!take || im == im0)) {
                        const float v = cl_wave_sum(take ? da : 0.0f);
                        if (lane == 0) atomicAdd(A.d_img + (im0 - 1), v);
                    } else {
                        cl_image_grad_segments(A.d_img, im, da, take, lane);
                    }
                }
            }
        }
    }
    __shared__ double sh[SPRIOR_T / 64];
    acc = wave_sum_d(acc);
    if (lane == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) A.kl_part[blockIdx.x] = ((sh[0] + sh[1]) + (sh[2] + sh[3])) * (double)w;
}

// the workgroups' partials, added up by one wave in a fixed order: lane l takes parts l, l + 64, ... in index order, then the wave's tree
__global__ __launch_bounds__(64) void scale_kl_sum_kernel(const double* __restrict__ part, int nparts, double* __restrict__ value, int accumulate,
                                                          const int* stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    double s = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 64) s += part[k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) *value = (accumulate ? *value : 0.0) + s;
}

// the step's record (behind cl_step_finalize): the term in the sixth double, and in the loss of a step that was not skipped
__global__ void scale_kl_record_kernel(const double* __restrict__ value, double* __restrict__ history, int step_index) {
    double* rec = history + (size_t)step_index * CL_HIST_STRIDE;
    if (rec[4] != 0.0) { rec[5] = 0.0; return; }
    const double v = *value;
    rec[5] = v;
    rec[0] += v;
}

inline int sprior_grid(long long n) {
    long long g = (n + SPRIOR_T - 1) / SPRIOR_T;
    if (g > CL_LAUE_LIK_MAX_BLOCKS) g = CL_LAUE_LIK_MAX_BLOCKS;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" {

int cl_scale_kl_grid(long long n) { return n < 1 ? 0 : sprior_grid(n); }

int cl_scale_kl(const cl_sprior_args* a, void* stream) {
    if (a == nullptr || a->loc == nullptr || a->sigma == nullptr || a->dO == nullptr || a->kl_part == nullptr || a->value == nullptr || a->n < 1) return -1;
    if (a->form != CL_SPRIOR_ANALYTIC && a->form != CL_SPRIOR_SAMPLE) return -1;
    if (a->kind != CL_SPRIOR_NORMAL && a->kind != CL_SPRIOR_LAPLACE && a->kind != CL_SPRIOR_STUDENTT) return -1;
    if (!(a->p_scale > 0.0f) || (a->kind == CL_SPRIOR_STUDENTT && !(a->p_df > 0.0f))) return -1;
    if (a->form == CL_SPRIOR_SAMPLE) {
        if (a->S < 1) return -1;
        if (a->use_img && (a->image_id == nullptr || a->img == nullptr || (a->d_img == nullptr && a->dimg_obs == nullptr))) return -1;
    } else if (a->kind != CL_SPRIOR_NORMAL || a->has_shift || a->use_img) {
        return -2;           // TFP registers a KL for a bare Normal against a Normal only: everything else is the sample form
    }
    float t_const = 0.0f;
    if (a->kind == CL_SPRIOR_STUDENTT) {         // lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2, as cl_ref_prior's
        const double nu = (double)a->p_df;
        t_const = (float)(lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846));
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = sprior_grid(a->n);
    if (int e = cl_launch<scale_kl_kernel>(dim3(G), dim3(SPRIOR_T), st, *a, t_const)) return e;
    return cl_launch<scale_kl_sum_kernel>(dim3(1), dim3(64), st, (const double*)a->kl_part, G, a->value, a->accumulate, a->stop_flag);
}

int cl_scale_kl_record(const double* value, double* history, int step_index, void* stream) {
    if (value == nullptr || history == nullptr || step_index < 0) return -1;
    return cl_launch<scale_kl_record_kernel>(dim3(1), dim3(1), (hipStream_t)stream, value, history, step_index);
}

}  // extern "C"
