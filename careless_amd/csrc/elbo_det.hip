// Deterministic mode (gfx950; include/careless_hip.h: cl_det_args): fixed-order sums of the per-observation stores of elbo_mlp.hip
// (-DCL_DET=1) and of cl_slot_rows / cl_laue_likelihood's deterministic forms.  Direct tests: tests/test_rows_kernels_gpu.py.
#include <hip/hip_runtime.h>
#include "cl_kernels.h"

// dz_f[r][s] += sum over the observations of reflection r in a FIXED order: sixteen lanes share a reflection -- lane l takes the rows
// l, l + 16, ... of its (row-ordered) list, the sixteen lane sums combine in a fixed butterfly.  (Round 3 walked the list with one
// thread per (reflection, sample): ~30 dependent random 4-byte gathers per thread, 0.39 ms per step at 10 M observations -- a fifth of
// the default scaler's step; the order of the sum is as fixed this way, and the gathers of a reflection are in flight together.)
__global__ __launch_bounds__(256) void det_refl_kernel(const cl_det_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int sub = threadIdx.x & 15;
    const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool on = r < A.R;
    const int k0 = on ? A.seg_refl[r] : 0, k1 = on ? A.seg_refl[r + 1] : 0;
    // the sixteen lanes of a reflection = (row slot, sample): the S' = 1, 2, 4, 8 or 16 samples of a row are consecutive lanes (a row's
    // record is S consecutive floats: one request), 16 / S' rows are in flight per pass; more than 16 samples go in chunks of 16
    const int Sp = A.S <= 1 ? 1 : (A.S <= 2 ? 2 : (A.S <= 4 ? 4 : (A.S <= 8 ? 8 : 16)));
    const int ss = sub & (Sp - 1), slot = sub / Sp, nslot = 16 / Sp;
    for (int s0 = 0; s0 < A.S; s0 += 16) {
        const int s = s0 + ss;
        float acc = 0.0f;
        if (s < A.S) {
            if (A.perm_refl != nullptr) {
                for (int k = k0 + slot; k < k1; k += nslot) acc += A.dzf_obs[(size_t)A.perm_refl[k] * A.S + s];
            } else {            // the records were stored in reflection order (cl_mlp_args.det_slot): a contiguous read
                for (int k = k0 + slot; k < k1; k += nslot) acc += A.dzf_obs[(size_t)k * A.S + s];
            }
        }
        for (int off = 8; off >= Sp; off >>= 1) acc += __shfl_xor(acc, off);      // over the row slots, fixed order
        if (on && slot == 0 && s < A.S) A.dz_f[(size_t)r * A.S + s] += acc;
    }
}

// d_img[m - 1] += sum over the observations of image m (m >= 1), one wave per image: lane l takes the rows l, l + 64, ... of the
// image's range in order, the 64 lane sums combine in a fixed butterfly
__global__ __launch_bounds__(256) void det_img_kernel(const cl_det_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int m = 1 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= A.n_images) return;
    float acc = 0.0f;
    for (int k = A.seg_img[m] + lane; k < A.seg_img[m + 1]; k += 64) acc += A.dimg_obs[A.perm_img[k]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) A.d_img[m - 1] += acc;
}

// scalars[NLL] += the workgroups' NLL in index order (one wave; lane l sums parts l, l + 64, ..., then the fixed butterfly)
__global__ __launch_bounds__(64) void det_nll_kernel(const cl_det_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    double acc = 0.0;
    for (int k = threadIdx.x; k < A.nparts; k += 64) acc += A.nll_part[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (threadIdx.x == 0) A.scalars[CL_SC_NLL] += acc;
}

// d_ev11[c] += the waves' shares of dL/d raw (Evans-2011 error model) in slot order: one wave, lane l sums slots l, l + 64, ..., then the fixed butterfly
__global__ __launch_bounds__(64) void det_ev11_kernel(const cl_det_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int k = threadIdx.x; k < A.n_ev11; k += 64) { a0 += A.ev11_part[3 * k]; a1 += A.ev11_part[3 * k + 1]; a2 += A.ev11_part[3 * k + 2]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); }
    if (threadIdx.x == 0) { A.d_ev11[0] += a0; A.d_ev11[1] += a1; A.d_ev11[2] += a2; }
}

extern "C" int cl_det_reduce(const cl_det_args* a, void* stream) {
    if (a == nullptr || a->dzf_obs == nullptr || a->seg_refl == nullptr || a->dz_f == nullptr || a->R < 1 || a->S < 1 ||
        a->nll_part == nullptr || a->nparts < 1 || a->scalars == nullptr)
        return -1;
    if (a->d_img != nullptr && (a->dimg_obs == nullptr || a->perm_img == nullptr || a->seg_img == nullptr || a->n_images < 1)) return -1;
    if (a->ev11_part != nullptr && (a->d_ev11 == nullptr || a->n_ev11 < 1)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (a->ev11_part != nullptr)
        if (int e = cl_launch<det_ev11_kernel>(dim3(1), dim3(64), st, *a)) return e;
    if (int e = cl_launch<det_refl_kernel>(dim3((unsigned)((a->R + 15) / 16)), dim3(256), st, *a)) return e;
    if (a->d_img != nullptr && a->n_images > 1)
        if (int e = cl_launch<det_img_kernel>(dim3((a->n_images - 1 + 3) / 4), dim3(256), st, *a)) return e;
    return cl_launch<det_nll_kernel>(dim3(1), dim3(64), st, *a);
}
