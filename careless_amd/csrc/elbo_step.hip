// The optimizer half of the ELBO step (gfx950; include/careless_hip.h: "gradient norm, sanitise, clip, Adam"): HBM-streaming, one pass each.
//
//   grad_sqnorm_kernel      global (and per-tensor) squared L2 norm of the flat gradient   [variational.py:205]
//   owner_qnorm_kernel      a rank's own share of the surrogate-posterior gradient's norm (reflection-owner data parallelism)
//   adam_kernel             non-finite -> 0, optional clipping, tf_keras Adam update       [variational.py:208-209, manager.py:494-501]
//   finalize_kernel         per-step history record + the sticky stop flag               [variational.py:262-274]
//   reduce_partials_kernel  the per-workgroup partial rows of a launch summed in index order
// Each kernel is bandwidth-trivial next to the fused MLP kernel; they exist to keep the whole step on the device with no host round
// trip.  Compiled with NaNs honoured (build.py): the non-finite stop is taken on the norm.  Direct tests: tests/test_step_kernels.py.
#include <hip/hip_runtime.h>
#include "cl_kernels.h"

__device__ __forceinline__ int seg_of(const int* __restrict__ seg_off, int nseg, int i) {
    int lo = 0, hi = nseg;               // seg_off has nseg + 1 entries
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, int n, const int* __restrict__ seg_off,
                                                          int nseg, double* __restrict__ seg_sq, double* scalars,
                                                          const unsigned char* __restrict__ frozen, const int* stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    double acc = 0.0, sane = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        // (a tensor that is not trainable is not among the gradients the reference takes the norm of: tape.gradient(loss,
        //  self.trainable_variables), variational.py:201-205)
        if (frozen != nullptr && frozen[seg_of(seg_off, nseg, i)] != 0) continue;
        const float v = g[i];
        const double v2 = (double)v * (double)v;
        acc += v2;                                           // raw: a NaN gradient gives a NaN norm (variational.py:205)
        const double s2 = isfinite(v) ? v2 : 0.0;           // what the optimizer's clipping sees (after :208)
        sane += s2;
        if (seg_sq != nullptr) atomicAdd(seg_sq + seg_of(seg_off, nseg, i), s2);
    }
    block_atomic_add_d(acc, scalars + CL_SC_GNORM2);
    __syncthreads();
    block_atomic_add_d(sane, scalars + CL_SC_GNORM2_SANE);
}

// Reflection-owner data parallelism: squared norm of this rank's own part of the surrogate-posterior gradient -- d a and d b of
// reflections [r0, r1) -- as four floats of the step's message (raw, sanitised, sanitised per tensor).  Double accumulation through
// scratch[0..3]; the last workgroup to arrive (ticket in scratch[4]) converts.  The caller zeroes scratch once per step.
__global__ __launch_bounds__(256) void owner_qnorm_kernel(const float* __restrict__ g, int R, int r0, int r1, float* __restrict__ out,
                                                          double* scratch, const int* stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    const int nr = r1 - r0;
    double raw = 0.0, sa = 0.0, sb = 0.0;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < 2 * nr; t += gridDim.x * blockDim.x) {
        const bool isb = t >= nr;
        const float v = g[isb ? R + r0 + (t - nr) : r0 + t];
        const double v2 = (double)v * (double)v;
        raw += v2;
        const double s2 = isfinite(v) ? v2 : 0.0;
        if (isb) sb += s2; else sa += s2;
    }
    block_atomic_add_d(raw, scratch + 0);
    __syncthreads();
    block_atomic_add_d(sa, scratch + 2);
    __syncthreads();
    block_atomic_add_d(sb, scratch + 3);
    __shared__ unsigned last;
    if (threadIdx.x == 0) {
        // release / acquire at agent scope on the ticket: the block's three sums are visible to whoever draws the last ticket (on a
        // multi-XCD part relaxed ordering guarantees nothing across L2s).  At most 64 workgroups take a ticket, so the L2 write-back
        // the release implies costs microseconds at worst (the same fence per workgroup of a 1 221-workgroup launch: tn_forward
        // 20 -> 30 us, which is why the big launches store per-workgroup parts instead)
        last = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(scratch + 4), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (last == gridDim.x - 1 && threadIdx.x == 0) {
        const double qa = atomicAdd(scratch + 2, 0.0), qb = atomicAdd(scratch + 3, 0.0), qr = atomicAdd(scratch + 0, 0.0);
        scratch[1] = qa + qb;
        out[0] = (float)qr;
        out[1] = (float)(qa + qb);
        out[2] = (float)qa;
        out[3] = (float)qb;
    }
}

__global__ __launch_bounds__(256) void adam_kernel(const cl_adam_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    float gscale = 1.0f;
    if (A.global_clipnorm > 0.0f) {
        // tf.clip_by_global_norm over the sanitised gradients [3P]: g * clip / max(norm, clip)
        const float nrm = (float)sqrt(A.scalars[CL_SC_GNORM2_SANE]);
        gscale = A.global_clipnorm / fmaxf(nrm, A.global_clipnorm);
    }
    double acc = 0.0, sane = 0.0;
    // the indices this call updates: the whole vector, or (reflection-owner data parallelism) up to three ranges -- the rank's own
    // reflections' a and b, whose norm over all ranks arrives in norm_extra, and the replicated tail
    const int len0 = A.n_ranges > 0 ? A.range_end[0] - A.range_begin[0] : A.n;
    const int len1 = A.n_ranges > 1 ? A.range_end[1] - A.range_begin[1] : 0;
    const int len2 = A.n_ranges > 2 ? A.range_end[2] - A.range_begin[2] : 0;
    const int total = len0 + len1 + len2;
    if (A.norm_out != nullptr && A.norm_extra != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        acc = (double)A.norm_extra[0];
        sane = (double)A.norm_extra[1];
    }
    // Four elements per thread and round, all their loads issued before the first store: p / m / v / g may alias as far as the compiler
    // knows, so the one-element loop was a chain of dependent memory round trips (15 - 23 us for 6.4e5 parameters; the arithmetic is
    // nothing).  Elements of a round are a grid stride apart: coalesced as before.
    const int stride = gridDim.x * blockDim.x;
    constexpr int U = 4;
    for (int t0 = blockIdx.x * blockDim.x + threadIdx.x; t0 < total; t0 += U * stride) {
        int ii[U], rk[U];
        float g_[U], m_[U], v_[U], p_[U];
        bool on[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u * stride;
            on[u] = t < total;
            int i = on[u] ? t : 0, r = 0;
            if (A.n_ranges > 0 && on[u]) {
                if (t < len0) { i = A.range_begin[0] + t; }
                else if (t < len0 + len1) { i = A.range_begin[1] + (t - len0); r = 1; }
                else { i = A.range_begin[2] + (t - len0 - len1); r = 2; }
            }
            ii[u] = i; rk[u] = r;
            g_[u] = A.g[i]; m_[u] = A.m[i]; v_[u] = A.v[i]; p_[u] = A.p[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!on[u]) continue;
            const int i = ii[u];
            float g = g_[u];
            // (a frozen tensor is neither updated nor part of the norm: the reference's gradients are those of trainable_variables)
            if (A.frozen != nullptr && A.frozen[seg_of(A.seg_off, A.nseg, i)] != 0) continue;
            if (A.norm_out != nullptr && rk[u] >= A.norm_skip_ranges) {    // fused tf.linalg.global_norm (variational.py:205)
                const double v2 = (double)g * (double)g;
                acc += v2;
                sane += isfinite(g) ? v2 : 0.0;
            }
            if (!isfinite(g)) g = 0.0f;                                   // variational.py:208
            if (A.clipnorm > 0.0f) {                                      // per-tensor tf.clip_by_norm [3P]
                const float nrm = (float)sqrt(A.seg_sq[seg_of(A.seg_off, A.nseg, i)]);
                if (nrm > A.clipnorm) g *= A.clipnorm / nrm;
            }
            g *= gscale;
            if (A.clipvalue > 0.0f) g = fminf(fmaxf(g, -A.clipvalue), A.clipvalue);
            float m = m_[u], v = v_[u];
            m += (g - m) * (1.0f - A.beta1);
            v += (g * g - v) * (1.0f - A.beta2);
            A.m[i] = m;
            A.v[i] = v;
            A.p[i] = p_[u] - m * A.alpha / (sqrtf(v) + A.adam_eps);
        }
    }
    if (A.norm_out != nullptr && A.norm_part != nullptr) {
        // one store pair per workgroup; cl_step_finalize adds them up (the whole grid is resident at once: its same-address atomics
        // would queue up at the end of the kernel)
        __shared__ double sh[2][4];
        const double wa = wave_sum_d(acc), ws = wave_sum_d(sane);
        if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = wa; sh[1][threadIdx.x >> 6] = ws; }
        __syncthreads();
        if (threadIdx.x < 2) A.norm_part[2 * blockIdx.x + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
    } else if (A.norm_out != nullptr) {
        block_atomic_add_d(acc, A.norm_out + CL_SC_GNORM2);
        __syncthreads();
        block_atomic_add_d(sane, A.norm_out + CL_SC_GNORM2_SANE);
    }
}

// one wave: add up what cl_adam_step left per workgroup (norm_part), then lane 0 writes the history record of this step and updates
// the sticky stop flag
__global__ void finalize_kernel(double* scalars, float kl_weight_or_one, double* history, int step_index,
                                int hist_stride, int* stop_flag, const double* __restrict__ norm_part, int n_norm_part) {
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    double* rec = history + (size_t)step_index * hist_stride;
    if (stop_flag != nullptr && *stop_flag != 0) {
        if (threadIdx.x == 0) {
            rec[0] = rec[1] = rec[2] = rec[3] = 0.0;
            rec[4] = 1.0;                  // skipped
        }
        return;
    }
    double gn2 = scalars[CL_SC_GNORM2];
    if (norm_part != nullptr) {
        double a = 0.0, b = 0.0;
        for (int i = threadIdx.x; i < n_norm_part; i += 64) { a += norm_part[2 * i]; b += norm_part[2 * i + 1]; }
        a = wave_sum_d(a); b = wave_sum_d(b);
        gn2 += a;
        if (threadIdx.x == 0) { scalars[CL_SC_GNORM2] = gn2; scalars[CL_SC_GNORM2_SANE] += b; }
    }
    if (threadIdx.x != 0) return;
    const double nll = scalars[CL_SC_NLL], kl = scalars[CL_SC_KL];
    const double gn = sqrt(gn2);
    rec[0] = nll + (double)kl_weight_or_one * kl;   // loss
    rec[1] = kl;                                    // "F KLDiv"
    rec[2] = nll;                                   // "NLL"
    rec[3] = gn;                                    // "Grad Norm"
    rec[4] = 0.0;
    if (stop_flag != nullptr && !isfinite(gn)) *stop_flag = 1;     // variational.py:271-274
}

// sum of the per-workgroup partials of a scaler launch in a fixed order -> MLP slice of the flat gradient buffer (the work of a workgroup
// is cl_reduce_partials_block, cl_kernels.h: shared with the cl_tn_backward / cl_rw_backward launch, which can carry it)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partials, int nparts, int P,
                                                               float* __restrict__ out, const int* stop_flag) {
    if (stop_flag != nullptr && *stop_flag != 0) return;
    cl_reduce_partials_block(partials, nparts, P, out, (int)blockIdx.x);
}

// (unchecked: the tail of cl_peel_backward and cl_nlik_backward, which have checked their own arguments)
int cl_launch_reduce_partials(const float* partials, int nparts, int P, float* out, const int* stop_flag, hipStream_t st) {
    return cl_launch<reduce_partials_kernel>(dim3((P + 31) / 32), dim3(256), st, partials, nparts, P, out, stop_flag);
}

// workgroups of cl_adam_step (a -> n >= 1)
static int adam_grid(const cl_adam_args& a) {
    int work = a.n;
    if (a.n_ranges > 0) {
        work = 0;
        for (int k = 0; k < a.n_ranges; ++k) work += a.range_end[k] - a.range_begin[k];
        if (work < 1) work = 1;
    }
    int grid = (work + 1023) / 1024;          // four elements per thread and round
    // without norm_part a workgroup ends in two same-address fp64 atomics (fused gradient norm), ~12 ns each and serialised: few
    // workgroups then for the usual ~1e6 parameters, more when the vector is long enough for streaming to dominate (per-image layers:
    // 4e7 parameters)
    const int cap = (a.n >= (1 << 22) || a.norm_out == nullptr || a.norm_part != nullptr) ? 1024 : 256;
    if (grid > cap) grid = cap;
    return grid;
}

extern "C" {

int cl_reduce_partials(const float* partials, int nparts, int P, float* grad_mlp, const int* stop_flag, void* stream) {
    if (partials == nullptr || grad_mlp == nullptr || nparts < 1 || P < 1) return -1;
    return cl_launch_reduce_partials(partials, nparts, P, grad_mlp, stop_flag, (hipStream_t)stream);
}

int cl_grad_sqnorm(const float* g, int n, const int* seg_off, int nseg, double* seg_sq, double* scalars,
                   const unsigned char* frozen, const int* stop_flag, void* stream) {
    if (g == nullptr || scalars == nullptr || n < 1) return -1;
    if ((seg_sq != nullptr || frozen != nullptr) && (seg_off == nullptr || nseg < 1)) return -1;
    int grid = (n + 255) / 256;
    if (grid > 1024) grid = 1024;
    return cl_launch<grad_sqnorm_kernel>(dim3(grid), dim3(256), (hipStream_t)stream, g, n, seg_off, nseg, seg_sq, scalars, frozen, stop_flag);
}

int cl_adam_grid(const cl_adam_args* a) { return (a == nullptr || a->n <= 0) ? -1 : adam_grid(*a); }

int cl_adam_step(const cl_adam_args* a, void* stream) {
    if (a == nullptr || a->p == nullptr || a->g == nullptr || a->m == nullptr || a->v == nullptr || a->n < 1) return -1;
    if ((a->clipnorm > 0.0f || a->frozen != nullptr) && (a->seg_off == nullptr || a->nseg < 1)) return -1;
    if (a->clipnorm > 0.0f && a->seg_sq == nullptr) return -1;
    if (a->global_clipnorm > 0.0f && a->scalars == nullptr) return -1;
    if (a->n_ranges < 0 || a->n_ranges > 3 || a->norm_skip_ranges < 0 || a->norm_skip_ranges > a->n_ranges) return -1;
    for (int k = 0; k < a->n_ranges; ++k)
        if (a->range_begin[k] < 0 || a->range_end[k] > a->n || a->range_end[k] < a->range_begin[k]) return -1;
    return cl_launch<adam_kernel>(dim3(adam_grid(*a)), dim3(256), (hipStream_t)stream, *a);
}

int cl_owner_qnorm(const float* g, int R, int r_begin, int r_end, float* out, double* scratch, const int* stop_flag, void* stream) {
    if (g == nullptr || out == nullptr || scratch == nullptr || R < 1 || r_begin < 0 || r_end > R || r_end <= r_begin) return -1;
    int grid = (2 * (r_end - r_begin) + 1023) / 1024;
    if (grid > 64) grid = 64;
    if (grid < 1) grid = 1;
    return cl_launch<owner_qnorm_kernel>(dim3(grid), dim3(256), (hipStream_t)stream, g, R, r_begin, r_end, out, scratch, stop_flag);
}

int cl_step_finalize(double* scalars, float kl_weight_or_one, double* history, int step_index, int* stop_flag,
                     const double* norm_part, int n_norm_part, void* stream) {
    if (scalars == nullptr || history == nullptr || step_index < 0) return -1;
    if (norm_part != nullptr && n_norm_part < 1) return -1;
    return cl_launch<finalize_kernel>(dim3(1), dim3(64), (hipStream_t)stream, scalars, kl_weight_or_one, history, step_index, (int)CL_HIST_STRIDE,
                                      stop_flag, norm_part, n_norm_part);
}

}  // extern "C"
