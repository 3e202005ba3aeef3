// The text of the two surrogate-posterior kernels of csrc/elbo_q.hip, included there once per posterior: as tn_forward_kernel /
// tn_backward_kernel (truncated normal, argument cl_tn_args) and as rw_forward_kernel / rw_backward_kernel (Rice-Woolfson, argument cl_rw_args).
// Two expansions of one text, as elbo_frozen_rows.h, rather than a body function called from two kernels: the truncated-normal kernels
// must stay what they were, instruction for instruction (a shared body moved their reads of the launch geometry), under their old names.
// Workspace clearing, KL parts, owned range, prior arms, the ride-along reduction and the stop flag are this text's; the posterior
// (CL_Q_POST: tn_post / rw_post of elbo_q.hip) supplies load / sample / log_prob / grads.
//   #define CL_Q_FORWARD_KERNEL <name>   #define CL_Q_BACKWARD_KERNEL <name>   #define CL_Q_ARGS <kernel argument type>
//   #define CL_Q_TN(KA) <its cl_tn_args>   #define CL_Q_POST <posterior type>   #define CL_Q_POST_OF(KA) <the posterior of a launch>
__global__ __launch_bounds__(256) void CL_Q_FORWARD_KERNEL(const CL_Q_ARGS KA) {
    const cl_tn_args& A = CL_Q_TN(KA);
    CL_Q_POST q = CL_Q_POST_OF(KA);
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const bool part = A.r_end > A.r_begin;               // an owned reflection range (reflection-owner data parallelism)
    const int h = (part ? A.r_begin : 0) + blockIdx.x * blockDim.x + threadIdx.x;
    // the step's accumulators, cleared on the way (instead of a memset launch in front of this one): the flat gradient + scalar block
    // by all threads, the dz_f rows of this launch's reflections by their threads
    if (A.zero_ptr != nullptr) {
        const long long n4 = A.zero_n >> 2;              // (16-byte aligned, a multiple of four floats: the caller's workspace layout)
        f32x4_t* z4 = reinterpret_cast<f32x4_t*>(A.zero_ptr);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) z4[i] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
        for (long long i = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.zero_n; i += (long long)gridDim.x * blockDim.x) A.zero_ptr[i] = 0.0f;
    }
    double kl = 0.0;
    if (h < (part ? A.r_end : A.R)) {
        if (A.zero_dzf != nullptr)
            for (int s = 0; s < A.S; ++s) A.zero_dzf[(size_t)h * A.S + s] = 0.0f;
        const float a = A.q_loc_raw[h], b = A.q_scale_raw[h];
        q.load(A, h);
        const bool in_kl = (h >= A.kl_begin && h < A.kl_end);
        const bool dw_child = (A.prior_kind == CL_PRIOR_DOUBLE_WILSON_) && (A.root[h] == 0);
        cl_u32x4 blk = {};
        for (int s = 0; s < A.S; ++s) {
            const CL_Q_POST::elem t = q.sample(A, a, b, h, s, blk);
            A.z_f[(size_t)h * A.S + s] = t.z;
            if (in_kl) {
                float dlp;
                const float lq = CL_Q_POST::log_prob(t);
                // non-root reflections of a double-Wilson model get their conditional prior in dw_forward_kernel (needs z_parent), every
                // reflection of a reference-prior model in ref_prior_kernel
                const float lp = (dw_child || A.prior_kind == CL_PRIOR_REFERENCE_) ? 0.0f : prior_lp(A, h, t.z, &dlp);
                kl += (double)(lq - lp);
            }
        }
    }
    if (A.kl_part != nullptr) {
        // one store per workgroup; the step's cl_tn_backward adds the parts up (no atomics, fixed order)
        __shared__ double sh[4];
        const double w = wave_sum_d(kl * (double)A.w_kl);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) A.kl_part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    } else {
        block_atomic_add_d(kl * (double)A.w_kl, A.scalars + CL_SC_KL);
    }
}

__global__ __launch_bounds__(256) void CL_Q_BACKWARD_KERNEL(const CL_Q_ARGS KA) {
    const cl_tn_args& A = CL_Q_TN(KA);
    CL_Q_POST q = CL_Q_POST_OF(KA);
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const bool part = A.r_end > A.r_begin;
    const int nb_tn = ((part ? A.r_end - A.r_begin : A.R) + 255) / 256;      // workgroups of the reflections; the rest carry the reduction
    if ((int)blockIdx.x >= nb_tn) {
        cl_reduce_partials_block(A.red_partials, A.red_nparts, A.red_P, A.red_out, (int)blockIdx.x - nb_tn);
        return;
    }
    if (A.kl_part != nullptr && blockIdx.x == 0) {
        // the KL sums the forward launch(es) left per workgroup (same grid; the double-Wilson pass always covers all R): added up
        // here, in index order
        const int nb = nb_tn;
        double t = 0.0;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) t += A.kl_part[i];
        if (A.kl_part_dw != nullptr && (A.prior_kind == CL_PRIOR_DOUBLE_WILSON_ || A.prior_kind == CL_PRIOR_REFERENCE_))
            for (int i = threadIdx.x; i < (A.R + 255) / 256; i += blockDim.x) t += A.kl_part_dw[i];
        __shared__ double sh[4];
        const double w = wave_sum_d(t);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) A.scalars[CL_SC_KL] += (sh[0] + sh[1]) + (sh[2] + sh[3]);
    }
    const int h = (part ? A.r_begin : 0) + blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= (part ? A.r_end : A.R)) return;
    const float a = A.q_loc_raw[h], b = A.q_scale_raw[h];
    q.load(A, h);
    const bool in_kl = (h >= A.kl_begin && h < A.kl_end);
    const float wkl = in_kl ? A.w_kl * A.kl_grad_mult : 0.0f;
    const bool dw_child = (A.prior_kind == CL_PRIOR_DOUBLE_WILSON_) && (A.root[h] == 0);
    float gloc = 0.0f, gscale = 0.0f, loc = 0.0f, scale = 0.0f;
    cl_u32x4 blk = {};
    for (int s = 0; s < A.S; ++s) {
        const CL_Q_POST::elem t = q.sample(A, a, b, h, s, blk);
        loc = t.loc; scale = t.scale;
        float dq_dz, dq_dloc, dq_dscale, dp_dz;
        CL_Q_POST::grads(t, &dq_dz, &dq_dloc, &dq_dscale);
        if (dw_child) {
            const int par = A.parent_ids[h];
            const float zp = (par >= 0) ? A.z_f[(size_t)par * A.S + s] : 0.0f;
            float dzp, dr;
            (void)cl_dw_log_prob(t.z, zp, par >= 0, dw_r_of(A, h), A.centric[h] != 0, A.es[h], &dp_dz, &dzp, &dr);
        } else if (A.prior_kind == CL_PRIOR_REFERENCE_) {
            dp_dz = 0.0f;               // (ref_prior_kernel has added the prior's z-derivative to dz_f)
        } else {
            (void)prior_lp(A, h, t.z, &dp_dz);
        }
        const float gz = A.dz_f[(size_t)h * A.S + s] + wkl * (dq_dz - dp_dz);
        gloc += gz * t.dz_dloc + wkl * dq_dloc;
        gscale += gz * t.dz_dscale + wkl * dq_dscale;
    }
    // raw parameters: loc = exp(a), scale = exp(b) + eps
    A.d_loc_raw[h] += gloc * loc;
    A.d_scale_raw[h] += gscale * (scale - A.eps);
}
