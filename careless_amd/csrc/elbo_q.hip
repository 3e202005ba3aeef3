// Surrogate posterior and priors of the ELBO step (gfx950; include/careless_hip.h: "surrogate posterior + prior", "empirical reference
// priors", "Rice-Woolfson surrogate posterior"): per-reflection kernels, HBM-streaming, one pass each.
//
//   tn_forward_kernel     q(F) parameter transform + reparameterised truncated-normal sample z_f (S,R), and the
//                         sample-based KL partial sums  sum_s [log q(z) - log p(z)]
//                         [surrogate_posteriors.py:50-53,104-131; variational.py:123-139,154,173; wilson.py:50-57]
//   tn_backward_kernel    chain rule from dL/dz_f (data term, accumulated by the fused MLP kernel) plus the KL
//                         term's own derivatives back to the raw q parameters (a = log loc, b = log(scale - eps))
//   rw_forward_kernel /   the same two for the Rice-Woolfson posterior (Rice per acentric, folded normal per centric reflection): one text
//   rw_backward_kernel    (elbo_q_kernels.h, expanded twice), two posteriors   [surrogate_posteriors.py:133-172; distributions.py:228-348]
//   dw_forward_kernel /   the double-Wilson prior's conditional term of the non-root reflections, and its deterministic-mode pull
//   dw_parent_pull_kernel [wilson.py:146-175]
//   ref_prior_kernel      an empirical reference prior's -log p(z_f) into the KL and its z-derivative onto dL/dz_f, between the two
//                         [priors/empirical.py:9-131; variational.py:123-139]
// Each kernel is bandwidth-trivial next to the fused MLP kernel (R = N/32); they exist to keep the whole step on the device with no host
// round trip.  Direct tests: tests/test_q_kernels_gpu.py, tests/test_ref_prior_gpu.py, tests/test_rw_posterior_gpu.py.
#include <hip/hip_runtime.h>
#include "cl_math.h"
#include "cl_kernels.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// uniform of (reflection h, sample s); `blk` caches the Philox block shared by samples 4k .. 4k+3 across loop iterations
__device__ __forceinline__ float tn_uniform(const cl_tn_args& A, int h, int s, cl_u32x4& blk) {
    if (A.u_f) return A.u_f[(size_t)h * A.S + s];
    if ((s & 3) == 0) blk = cl_noise_uniform_block(A.seed, A.step, (uint32_t)s >> 2, (uint64_t)h);
    return cl_noise_uniform_pick(blk, (uint32_t)s);
}

// correlation r of reflection h with its parent: fixed (dw_r) or sigmoid of the trainable per-ASU value
__device__ __forceinline__ float dw_r_of(const cl_tn_args& A, int h) {
    return A.dw_r_raw ? cl_sigmoid(A.dw_r_raw[A.asu_ids[h]]) : A.dw_r[h];
}

// log-density of the Wilson prior and its z-derivative for reflection h
__device__ __forceinline__ float prior_lp(const cl_tn_args& A, int h, float z, float* dlp_dz) {
    const bool c = A.centric[h] != 0;
    const float es = A.es[h];
    *dlp_dz = cl_wilson_dlog_prob_dz(z, c, es);
    return cl_wilson_log_prob(z, c, es);
}

// What the kernel text of elbo_q_kernels.h asks of a posterior: `load` the reflection's constants, `sample` element (h, s) from injected or
// in-kernel noise (the backward pass redraws the forward pass' numbers), the element's log-density and its partial derivatives.
struct tn_post {
    typedef cl_tn_elem elem;
    float low;
    __device__ __forceinline__ void load(const cl_tn_args& A, int h) { low = A.low[h]; }
    __device__ __forceinline__ elem sample(const cl_tn_args& A, float a, float b, int h, int s, cl_u32x4& blk) const {
        return cl_tn_sample(a, b, low, A.high, A.eps, tn_uniform(A, h, s, blk));
    }
    static __device__ __forceinline__ float log_prob(const elem& t) { return cl_tn_log_prob(t); }
    static __device__ __forceinline__ void grads(const elem& t, float* dz, float* dloc, float* dscale) { cl_tn_log_prob_grads(t, dz, dloc, dscale); }
};

struct rw_post {
    typedef cl_rw_elem elem;
    const unsigned char* q_centric;
    const float* n_f;                    // [2][R][S] or NULL
    bool centric;
    __device__ __forceinline__ void load(const cl_tn_args&, int h) { centric = q_centric[h] != 0; }
    // `blk` caches the Philox block shared by samples 2k and 2k + 1 across loop iterations
    __device__ __forceinline__ elem sample(const cl_tn_args& A, float a, float b, int h, int s, cl_u32x4& blk) const {
        float n1, n2;
        if (n_f) {
            const size_t i = (size_t)h * A.S + s;
            n1 = n_f[i];
            n2 = n_f[(size_t)A.R * A.S + i];
        } else {
            if ((s & 1) == 0) blk = cl_noise_rw_block(A.seed, A.step, (uint32_t)s, (uint64_t)h);
            cl_noise_rw_pick(blk, (uint32_t)s, &n1, &n2);
        }
        return cl_rw_sample(a, b, A.eps, centric, n1, n2);
    }
    static __device__ __forceinline__ float log_prob(const elem& t) { return cl_rw_log_prob(t); }
    static __device__ __forceinline__ void grads(const elem& t, float* dz, float* dloc, float* dscale) { cl_rw_log_prob_grads(t, dz, dloc, dscale); }
};

}  // namespace

#define CL_Q_FORWARD_KERNEL tn_forward_kernel
#define CL_Q_BACKWARD_KERNEL tn_backward_kernel
#define CL_Q_ARGS cl_tn_args
#define CL_Q_TN(KA) KA
#define CL_Q_POST tn_post
#define CL_Q_POST_OF(KA) tn_post{}
#include "elbo_q_kernels.h"
#undef CL_Q_FORWARD_KERNEL
#undef CL_Q_BACKWARD_KERNEL
#undef CL_Q_ARGS
#undef CL_Q_TN
#undef CL_Q_POST
#undef CL_Q_POST_OF
#define CL_Q_FORWARD_KERNEL rw_forward_kernel
#define CL_Q_BACKWARD_KERNEL rw_backward_kernel
#define CL_Q_ARGS cl_rw_args
#define CL_Q_TN(KA) KA.tn
#define CL_Q_POST rw_post
#define CL_Q_POST_OF(KA) rw_post{KA.q_centric, KA.n_f, false}
#include "elbo_q_kernels.h"
#undef CL_Q_FORWARD_KERNEL
#undef CL_Q_BACKWARD_KERNEL
#undef CL_Q_ARGS
#undef CL_Q_TN
#undef CL_Q_POST
#undef CL_Q_POST_OF

// Double-Wilson conditional prior of the non-root reflections: -log p(z_h | z_parent) into the KL, and its derivative
// w.r.t. the parent's sample scattered into dz_f (the child's own derivative is taken in tn_backward_kernel).
__global__ __launch_bounds__(256) void dw_forward_kernel(const cl_tn_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    double kl = 0.0;
    float gr = 0.0f;                     // dL/dr of this reflection (trainable r only)
    int asu = -1;
    if (h < A.R && A.root[h] == 0 && h >= A.kl_begin && h < A.kl_end) {
        const int par = A.parent_ids[h];
        const float r = dw_r_of(A, h), es = A.es[h];
        const bool c = A.centric[h] != 0;
        const float wg = A.w_kl * A.kl_grad_mult;
        for (int s = 0; s < A.S; ++s) {
            const float z = A.z_f[(size_t)h * A.S + s];
            const float zp = (par >= 0) ? A.z_f[(size_t)par * A.S + s] : 0.0f;
            float dz, dzp, dr;
            const float lp = cl_dw_log_prob(z, zp, par >= 0, r, c, es, &dz, &dzp, &dr);
            kl -= (double)lp;
            gr -= wg * dr;
            if (par >= 0 && A.dw_child_seg == nullptr) atomicAdd(A.dz_f_out + (size_t)par * A.S + s, -wg * dzp);      // (deterministic mode: dw_parent_pull_kernel)
        }
        if (A.dw_r_raw) { asu = A.asu_ids[h]; gr *= r * (1.0f - r); }      // d sigmoid(raw) / d raw
    }
    if (A.dw_r_raw) {
        // reflections are ordered by ASU, so a wave almost always holds one ASU: wave-reduce, one atomic per wave
        const int a0 = __builtin_amdgcn_readfirstlane(asu);
        if (__all(asu == a0 || asu < 0)) {
            float v = (asu >= 0) ? gr : 0.0f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            const int any = __builtin_amdgcn_readfirstlane(__any(asu >= 0) ? 1 : 0);
            // a0 may be -1 when lane 0 is inactive: take the ASU of the first active lane instead
            int au = asu;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) au = max(au, __shfl_xor(au, off));
            if (any && (threadIdx.x & 63) == 0) atomicAdd(A.d_dw_r_raw + au, v);
        } else if (asu >= 0) {
            atomicAdd(A.d_dw_r_raw + asu, gr);
        }
    }
    if (A.kl_part_dw != nullptr && A.kl_part != nullptr) {          // (kl_part: the step's cl_tn_backward will add the parts up)
        __shared__ double sh[4];
        const double w = wave_sum_d(kl * (double)A.w_kl);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) A.kl_part_dw[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    } else {
        block_atomic_add_d(kl * (double)A.w_kl, A.scalars + CL_SC_KL);
    }
}

// Deterministic mode of the double-Wilson prior: what dw_forward_kernel's children scatter into their parents with float atomics, pulled
// by the parent instead -- thread p walks its children (CSR list, ascending) and adds -w dlogp(z_child | z_p) / dz_p to dz_f[p][s] in
// list order (recomputed: the term needs both samples, which are final).  Only children whose KL this rank owns count (row split).
__global__ __launch_bounds__(256) void dw_parent_pull_kernel(const cl_tn_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.R) return;
    const int k0 = A.dw_child_seg[p], k1 = A.dw_child_seg[p + 1];
    if (k1 <= k0) return;
    const float wg = A.w_kl * A.kl_grad_mult;
    for (int s = 0; s < A.S; ++s) {
        const float zp = A.z_f[(size_t)p * A.S + s];
        float acc = 0.0f;
        for (int k = k0; k < k1; ++k) {
            const int h = A.dw_child_ids[k];
            if (A.root[h] != 0 || h < A.kl_begin || h >= A.kl_end) continue;
            float dz, dzp, dr;
            (void)cl_dw_log_prob(A.z_f[(size_t)h * A.S + s], zp, true, dw_r_of(A, h), A.centric[h] != 0, A.es[h], &dz, &dzp, &dr);
            acc += -wg * dzp;
        }
        A.dz_f_out[(size_t)p * A.S + s] += acc;
    }
}

// Empirical reference prior (include/careless_hip.h: cl_ref_prior): thread per reflection, loop over S, like dw_forward_kernel -- but the
// density depends on the reflection's own sample only: the thread owns dz_f[h][.] (a plain read-modify-write, no atomic; the stream orders it
// behind the data term).  t_const: the Student-t density's constant, from the entry point.
__global__ __launch_bounds__(256) void ref_prior_kernel(const cl_refprior_args A, const float t_const) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    double kl = 0.0;
    if (h < A.R && h >= A.kl_begin && h < A.kl_end && (A.observed == nullptr || A.observed[h] != 0)) {
        const float loc = A.loc[h], scale = A.scale[h];
        const bool c = (A.kind == CL_REFPRIOR_RICE_WOOLFSON) && A.centric[h] != 0;
        const float wg = A.w_kl * A.kl_grad_mult;
        for (int s = 0; s < A.S; ++s) {
            const size_t i = (size_t)h * A.S + s;
            float dz;
            const float lp = cl_ref_prior_log_prob(A.kind, A.z_f[i], loc, scale, c, A.dof, t_const, &dz);
            kl -= (double)lp;
            A.dz_f[i] += -wg * dz;
        }
    }
    if (A.kl_part != nullptr) {
        // one store per workgroup, as tn_forward_kernel: the step's cl_tn_backward adds the parts up (no atomics, fixed order)
        __shared__ double sh[4];
        const double w = wave_sum_d(kl * (double)A.w_kl);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) A.kl_part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    } else {
        block_atomic_add_d(kl * (double)A.w_kl, A.scalars + CL_SC_KL);
    }
}

// ---------------------------------------------------------------------------------------------------------
// entry points: the argument check, then the launch
// ---------------------------------------------------------------------------------------------------------
// `need_low`: the truncated normal reads its lower bound; the Rice-Woolfson posterior (cl_rw_*) has none
static int check_tn(const cl_tn_args* a, bool need_low = true) {
    if (a == nullptr || a->q_loc_raw == nullptr || a->q_scale_raw == nullptr || (need_low && a->low == nullptr) || a->R < 1 || a->S < 1) return -1;
    // (a reference prior's term is cl_ref_prior's: the Wilson arrays are not read)
    if (a->prior_kind != CL_PRIOR_REFERENCE_ && (a->centric == nullptr || a->es == nullptr)) return -1;
    if (a->prior_kind == CL_PRIOR_DOUBLE_WILSON_ && (a->parent_ids == nullptr || a->root == nullptr)) return -1;
    if (a->prior_kind == CL_PRIOR_DOUBLE_WILSON_ && a->dw_r == nullptr && (a->dw_r_raw == nullptr || a->asu_ids == nullptr)) return -1;
    if (a->prior_kind != CL_PRIOR_DOUBLE_WILSON_ && a->prior_kind != CL_PRIOR_WILSON_ && a->prior_kind != CL_PRIOR_REFERENCE_) return -1;
    if (a->r_end > a->r_begin && (a->r_begin < 0 || a->r_end > a->R)) return -1;
    // an owned reflection range and the double-Wilson prior do not go together: a child's parent may belong to another rank
    if (a->r_end > a->r_begin && a->prior_kind == CL_PRIOR_DOUBLE_WILSON_) return -2;
    return 0;
}

// what the forward / backward launch of either posterior asks of the shared argument block, beyond check_tn
static int check_q_forward(const cl_tn_args* a) {
    if (a->z_f == nullptr || a->scalars == nullptr) return -1;
    if (a->zero_ptr != nullptr && (a->zero_n < 1 || (reinterpret_cast<uintptr_t>(a->zero_ptr) & 15) != 0)) return -1;
    // the KL must not be added into a block this launch is clearing: the parts go to kl_part then
    if (a->zero_ptr != nullptr && a->kl_part == nullptr) return -1;
    return 0;
}
static int check_q_backward(const cl_tn_args* a) {
    if (a->dz_f == nullptr || a->d_loc_raw == nullptr || a->d_scale_raw == nullptr) return -1;
    if (a->red_partials != nullptr && (a->red_out == nullptr || a->red_nparts < 1 || a->red_P < 1)) return -1;
    return 0;
}

// workgroups of a forward launch: the owned range, or all R reflections; a backward launch can carry a reduction on extra workgroups
static dim3 q_grid(const cl_tn_args& a, bool backward) {
    const int nr = a.r_end > a.r_begin ? a.r_end - a.r_begin : a.R;
    const int nred = (backward && a.red_partials != nullptr) ? (a.red_P + 31) / 32 : 0;
    return dim3((nr + 255) / 256 + nred);
}

extern "C" {

int cl_tn_forward(const cl_tn_args* a, void* stream) {
    if (int e = check_tn(a)) return e;
    if (int e = check_q_forward(a)) return e;
    return cl_launch<tn_forward_kernel>(q_grid(*a, false), dim3(256), (hipStream_t)stream, *a);
}

int cl_tn_backward(const cl_tn_args* a, void* stream) {
    if (int e = check_tn(a)) return e;
    if (int e = check_q_backward(a)) return e;
    return cl_launch<tn_backward_kernel>(q_grid(*a, true), dim3(256), (hipStream_t)stream, *a);
}

// Rice-Woolfson posterior (replaces reference surrogate_posteriors.py:133-172 on distributions.py:228-348; include/careless_hip.h: cl_rw_args)
int cl_rw_forward(const cl_rw_args* a, void* stream) {
    if (a == nullptr || a->q_centric == nullptr) return -1;
    if (int e = check_tn(&a->tn, false)) return e;
    if (int e = check_q_forward(&a->tn)) return e;
    return cl_launch<rw_forward_kernel>(q_grid(a->tn, false), dim3(256), (hipStream_t)stream, *a);
}

int cl_rw_backward(const cl_rw_args* a, void* stream) {
    if (a == nullptr || a->q_centric == nullptr) return -1;
    if (int e = check_tn(&a->tn, false)) return e;
    if (int e = check_q_backward(&a->tn)) return e;
    return cl_launch<rw_backward_kernel>(q_grid(a->tn, true), dim3(256), (hipStream_t)stream, *a);
}

int cl_dw_prior_forward(const cl_tn_args* a, void* stream) {
    if (int e = check_tn(a)) return e;
    if (a->prior_kind != CL_PRIOR_DOUBLE_WILSON_ || a->z_f == nullptr || a->dz_f_out == nullptr || a->scalars == nullptr) return -1;
    if (a->dw_r_raw != nullptr && (a->d_dw_r_raw == nullptr || a->n_asu < 1)) return -1;
    if ((a->dw_child_seg != nullptr) != (a->dw_child_ids != nullptr)) return -1;
    if (a->dw_child_seg != nullptr && a->dw_r_raw != nullptr) return -2;          // deterministic mode: fixed r only
    const dim3 grid((a->R + 255) / 256);
    if (int e = cl_launch<dw_forward_kernel>(grid, dim3(256), (hipStream_t)stream, *a)) return e;
    if (a->dw_child_seg == nullptr) return 0;
    return cl_launch<dw_parent_pull_kernel>(grid, dim3(256), (hipStream_t)stream, *a);
}

int cl_ref_prior(const cl_refprior_args* a, void* stream) {
    if (a == nullptr || a->z_f == nullptr || a->loc == nullptr || a->scale == nullptr || a->dz_f == nullptr || a->R < 1 || a->S < 1) return -1;
    if (a->kind < CL_REFPRIOR_NORMAL || a->kind > CL_REFPRIOR_RICE_WOOLFSON) return -1;
    if (a->kind == CL_REFPRIOR_STUDENTT && !(a->dof > 0.0f)) return -1;
    if (a->kind == CL_REFPRIOR_RICE_WOOLFSON && a->centric == nullptr) return -1;
    if (a->kl_part == nullptr && a->scalars == nullptr) return -1;
    float t_const = 0.0f;
    if (a->kind == CL_REFPRIOR_STUDENTT) {       // lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2, as the likelihood's lik_const
        const double nu = (double)a->dof;
        t_const = (float)(lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846));
    }
    return cl_launch<ref_prior_kernel>(dim3((a->R + 255) / 256), dim3(256), (hipStream_t)stream, *a, t_const);
}

}  // extern "C"
