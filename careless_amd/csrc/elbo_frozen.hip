// The data term of a step whose scaling model is FROZEN (gfx950 / CDNA4 only; round 6): `careless mono | poly --freeze-scales` and the
// half-dataset trainings of `--merge-half-datasets` (reference careless/careless.py:48-50, 102-128 -- as many steps again as the main
// training).  With the scaler frozen its output (loc, sigma) and the image scale of every observation are constants of the training:
// the caller takes them once (cl_mlp_forward / the wide path) and per step only what depends on the sampled amplitudes remains --
// sample the scale, predict, log-prob, gradient to dz_f and the Evans-2011 terms:
//   careless/models/merging/variational.py:156-181 (predict), models/likelihoods/mono.py:10-73 (log-prob), variational.py:197-202
//   (gradient of the trainable variables only: the scaler's is not taken).
//
// Round 5 ran this on cl_slot_rows (elbo_laue.hip): a thread per (row, sample) in the caller's row order and one memory-side float atomic
// of ~96 B per (row, sample) into dz_f -- 7 - 10 % of the HBM roof.  Here the CALLER sorts the rows by reflection once (the scaler's
// output is a constant: no tile, image or harmonic-group constraint binds the order) and
//   * a thread owns a ROW and loops over the samples: the row's seven numbers are read once (28 B, coalesced), one Philox block +
//     Box-Muller pair serves samples s and s + 4 as in the fused kernels (the noise is keyed by the row's GLOBAL number: bit for bit
//     the fused step's draws);
//   * the amplitude gradients of equal-reflection runs are summed inside the wave (rows are sorted: a run is a range of lanes; six
//     shuffle steps, the run's first lane ends with its total) and leave as ONE plain store per (reflection, sample) -- no atomics:
//     two runs of the same reflection can only meet at a wave boundary, those partial sums go to an edge buffer that a second small
//     launch adds up in wave order.  The step's data term is therefore DETERMINISTIC by construction;
//   * NLL in fp64 per workgroup, one atomic each (bounded grid), Evans-2011 gradients per wave.
// Roofline: HBM; algorithmic bytes per row 28 (+ 4 S per reflection, read and written once; + 4 S with injected noise).  With 8 samples
// the vector ALU (Philox + Box-Muller + Student-t per (row, sample)) is within a factor two of the HBM time: DESIGN 5.1b.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include "cl_math.h"
#include "cl_kernels.h"

namespace {

constexpr int FB = 256;                 // threads of a workgroup = rows of a chunk
// samples of a batch (registers): template parameter SB -- 1 for --mc-samples 1 (the default: no arrays of eight in the register
// budget, twice the waves per SIMD), 8 otherwise
constexpr int THROUGH = 1 << 30;        // edge_rid flag: the wave is ONE run that continues on both sides


}  // namespace

#define CL_FROZEN_ROWS_KERNEL frozen_rows_kernel
#define CL_FROZEN_ROWS_LAPLACE 0
#include "elbo_frozen_rows.h"
#undef CL_FROZEN_ROWS_KERNEL
#undef CL_FROZEN_ROWS_LAPLACE
#define CL_FROZEN_ROWS_KERNEL frozen_rows_laplace_kernel
#define CL_FROZEN_ROWS_LAPLACE 1
#include "elbo_frozen_rows.h"
#undef CL_FROZEN_ROWS_KERNEL
#undef CL_FROZEN_ROWS_LAPLACE

// Harmonic groups (Laue data, reference careless/models/likelihoods/laue.py:9-47: the predictions of the rows of one group SUM before the
// likelihood), first pass -- rows in the packed order of the single-pass kernels (obs.pack_laue: a group inside a 16-row granule, member
// index and size in gmeta, padding rows refl_id < 0), iobs / sig of the group replicated on its rows.  A thread owns a row and loops over
// the samples; the group's total comes over shuffles, every member evaluates the likelihood's derivative on it, member 0 counts the
// log-likelihood; the row's amplitude gradient is STORED at gbuf[row][s].  The rows of a group belong to different reflections, so one order
// cannot serve the group sums and the per-reflection sums: the second pass (frozen_rows_kernel with `src`) gathers gbuf in reflection order.
template <int SB, bool LAP>
__device__ __forceinline__ void frozen_laue_body(const cl_frozen_args& A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const int lane = threadIdx.x & 63;
    const int S = A.S;
    const long long n = A.n;
    const long long chunks = (n + FB - 1) / FB;
    double nll = 0.0;
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    cl_ev11 ev = {1.0f, 0.0f, 0.0f};
    const bool use_ev11 = A.ev11 != nullptr;
    if (use_ev11) { ev = cl_ev11_from_raw(A.ev11); }
    const float inv_dof = (A.lik_kind == CL_LIK_STUDENTT) ? 1.0f / A.dof : 0.0f;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long row = c * FB + threadIdx.x;
        const bool in = row < n;
        const long long rc = in ? row : n - 1;
        int rid = A.refl_id[rc];
        if (!in) rid = -1;
        const bool act = rid >= 0;
        const float loc = A.loc[rc], sigma = A.sigma[rc], io = A.iobs[rc], sg = A.sig[rc];
        const float aim = A.aim != nullptr ? A.aim[rc] : 1.0f;
        const long long key = A.key != nullptr ? (long long)A.key[rc] : A.obs_offset + row;
        // where this row's gradients go in gbuf: its position in REFLECTION order when the caller gives one (src: the second pass then reads
        // gbuf front to back -- a scattered 4 S-byte write per row here instead of a gathered 128-byte line per row there), else its own row
        const long long gdst = !in ? -1 : (A.src != nullptr ? (long long)A.src[rc] : row);
        const int gm = act ? A.gmeta[rc] : (1 << 8);
        const int mem = gm & 0xff, cnt = gm >> 8;
        int gmax = cnt;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gmax = max(gmax, __shfl_xor(gmax, off));
        gmax = __builtin_amdgcn_readfirstlane(gmax);
        const float inv_sg = cl_fast_rcp(sg), log_sg = cl_fast_log(sg);
        const float* __restrict__ eta_p = A.eta != nullptr ? A.eta + (size_t)(key - A.obs_offset) * S : nullptr;
        float* __restrict__ ip_p = A.ipred_out != nullptr ? A.ipred_out + (size_t)(key - A.obs_offset) * S : nullptr;
        const size_t zoff = (size_t)(act ? rid : 0) * S;
        for (int sb = 0; sb < S; sb += SB) {
            float e[SB];
            if (eta_p == nullptr) {
                if constexpr (SB == 1) {
                    float unused;
                    cl_noise_normal_pair(A.seed, A.step, 0u, (uint64_t)key, &e[0], &unused);
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        if (sb + p < S) cl_noise_normal_pair(A.seed, A.step, (uint32_t)(sb + p), (uint64_t)key, &e[p], &e[p + 4]);
                        else { e[p] = 0.0f; e[p + 4] = 0.0f; }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < SB; ++j) e[j] = (act && sb + j < S) ? eta_p[sb + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < SB; ++j) {
                if (sb + j < S) {                                  // (wave-uniform: every lane takes part in the shuffles)
                    const int s = sb + j;
                    const float zf = act ? A.z_f[zoff + s] : 0.0f;
                    const float tq = loc + sigma * e[j] + A.shift;
                    const float ipred = act ? aim * tq * zf * zf : 0.0f;
                    if (ip_p != nullptr && act) ip_p[s] = ipred;
                    float lin = 0.0f;
                    for (int mm = 0; mm < gmax; ++mm) {
                        const float v = __shfl(ipred, (lane - mem + mm) & 63);
                        lin += (mm < cnt) ? v : 0.0f;
                    }
                    float gj = 0.0f;
                    if (act) {
                        float dll, ll;
                        if (use_ev11) {
                            float gf, gb, ga;
                            ll = cl_lik_ev11(lin, io, sg, A.lik_kind, A.dof, A.lik_const, ev, &dll, &gf, &gb, &ga);
                            if (mem == 0) { g0 -= gf * A.w_ll; g1 -= ga * A.w_ll; g2 -= gb * A.w_ll; }
                        } else {
                            if constexpr (LAP) ll = cl_lik_laplace_log_prob2(lin, io, inv_sg, log_sg, &dll);
                            else ll = cl_lik_log_prob3(lin, io, inv_sg, log_sg, A.lik_kind, A.dof, inv_dof, A.lik_const, &dll);
                        }
                        if (mem == 0) nll -= (double)ll * (double)A.w_ll;
                        gj = -dll * A.w_ll * aim * tq * 2.0f * zf;
                    }
                    if (gdst >= 0) A.gbuf[(size_t)gdst * S + s] = gj;
                }
            }
        }
    }
    __shared__ double sh[FB / 64];
    nll = wave_sum_d(nll);
    if (lane == 0) sh[threadIdx.x >> 6] = nll;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < FB / 64; ++k) t += sh[k];
        if (A.nll_part != nullptr) A.nll_part[blockIdx.x] = t;
        else atomicAdd(A.scalars + CL_SC_NLL, t);
    }
    if (use_ev11) {
        g0 = cl_wave_sum(g0); g1 = cl_wave_sum(g1); g2 = cl_wave_sum(g2);
        if (lane == 0) {
            const float e0 = g0 * cl_sigmoid(A.ev11[0]), e1 = g1 * cl_sigmoid(A.ev11[1]), e2 = g2 * cl_sigmoid(A.ev11[2]);
            if (A.ev11_part != nullptr) {
                float* slot = A.ev11_part + 3 * ((FB / 64) * (size_t)blockIdx.x + (threadIdx.x >> 6));
                slot[0] = e0; slot[1] = e1; slot[2] = e2;
            } else { atomicAdd(A.d_ev11 + 0, e0); atomicAdd(A.d_ev11 + 1, e1); atomicAdd(A.d_ev11 + 2, e2); }
        }
    }
}

// The runs that cross wave borders: thread = (wave whose last run starts a chain, sample); it walks the chain in wave order -- the
// partial of that run, then the first-run partials of the following waves while they continue it -- and stores the total.
// frozen_laue_kernel with the likelihood kind picked at run time (Normal / Student-T) and its Laplace instance (cl_math.h says why the kind
// is not a third arm of cl_lik_log_prob3; frozen_rows_kernel's two expansions: elbo_frozen_rows.h)
template <int SB> __global__ __launch_bounds__(FB) void frozen_laue_kernel(const cl_frozen_args A) { frozen_laue_body<SB, false>(A); }
template <int SB> __global__ __launch_bounds__(FB) void frozen_laue_laplace_kernel(const cl_frozen_args A) { frozen_laue_body<SB, true>(A); }

__global__ __launch_bounds__(256) void frozen_edges_kernel(const cl_frozen_args A) {
    if (A.stop_flag != nullptr && *A.stop_flag != 0) return;
    const long long n_waves = (A.n + 63) / 64;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = A.S;
    if (t >= n_waves * S) return;
    const long long w = t / S;
    const int s = (int)(t - w * S);
    const int r = A.edge_rid[2 * w + 1];
    if (r < 0) return;
    float sum = A.edge_val[(size_t)(2 * w + 1) * S + s];
    for (long long j = w + 1; j < n_waves; ++j) {
        const int r0 = A.edge_rid[2 * j];
        if (r0 < 0 || (r0 & ~THROUGH) != r) break;
        sum += A.edge_val[(size_t)(2 * j) * S + s];
        if (!(r0 & THROUGH)) break;
    }
    if (A.accumulate) atomicAdd(A.dz_f + (size_t)r * S + s, sum);
    else A.dz_f[(size_t)r * S + s] = sum;
}

int cl_frozen_edge_floats(long long n, int S) { return (n <= 0 || S <= 0) ? 0 : (int)(2 * ((n + 63) / 64) * S); }
int cl_frozen_grid(long long n) {
    long long b = (n + FB - 1) / FB;
    if (b > CL_LAUE_LIK_MAX_BLOCKS) b = CL_LAUE_LIK_MAX_BLOCKS;
    return (int)(b < 1 ? 1 : b);
}

namespace {

// The three launches cl_frozen_rows serves (include/careless_hip.h: cl_frozen_args), told apart by gmeta / gbuf.
enum class frozen_form {
    ROWS,       // monochromatic rows sorted by reflection: likelihood, per-reflection sums, edges
    GROUPS,     // gmeta: harmonic groups in packed order, first call -- likelihood, per-row gradients into gbuf (no sums, no edges)
    SUMS,       // gbuf without gmeta: second call -- the stored gradients summed per reflection, edges (evaluates no likelihood)
};
frozen_form frozen_form_of(const cl_frozen_args& a) {
    return a.gmeta != nullptr ? frozen_form::GROUPS : a.gbuf != nullptr ? frozen_form::SUMS : frozen_form::ROWS;
}

// 0, or the negative code of the call -- every clause once, in the order that decides which code answers when several apply
int frozen_check(const cl_frozen_args& a, frozen_form f) {
    const bool lik = f != frozen_form::SUMS, edges = f != frozen_form::GROUPS;
    if (lik)
        if (int e = cl_lik_check(a.lik_kind, a.ev11, a.d_ev11, a.ev11_part, true)) return e;
    if (a.n <= 0 || a.S <= 0 || a.refl_id == nullptr) return -1;
    if (lik && any_null(a.loc, a.sigma, a.iobs, a.sig, a.z_f, a.scalars)) return -1;
    if (edges ? any_null(a.dz_f, a.edge_rid, a.edge_val) : a.gbuf == nullptr) return -1;        // (SUMS has its gbuf by definition)
    // the kernels' 32-bit row indices; a reflection id beside the THROUGH flag of edge_rid
    if (a.n >= (1ll << 31) - 64 || (edges && a.R >= THROUGH)) return -4;
    if (a.ev11 != nullptr && a.d_ev11 == nullptr && a.ev11_part == nullptr) return -1;
    return 0;
}

// Launch of the row-per-thread instance `Kern` over n rows on as many workgroups as the device holds at once (a grid-stride loop over
// equal shares: a second, partial round of workgroups would leave most of the device waiting for it), never more than cl_frozen_grid(n)
// (the size of nll_part / ev11_part).  The kernel is a template ARGUMENT, so the cache of its resident grid is one per instance (as
// cl_launch_lds' mark: cl_kernels.h).  One process drives one device: the cache is filled for the device current at the first call.
template <auto Kern>
int frozen_launch(const cl_frozen_args& a, hipStream_t st) {
    static std::atomic<int> resident{0};
    int g = resident.load(std::memory_order_relaxed), dev = 0, cus = 0, per = 0;
    if (g == 0 && hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, Kern, FB, 0) == hipSuccess && per >= 1 && cus >= 1)
        resident.store(g = per * cus, std::memory_order_relaxed);
    const int cap = cl_frozen_grid(a.n);
    return cl_launch<Kern>(dim3((unsigned)(g > 0 && g < cap ? g : cap)), dim3(FB), st, a);
}

}  // namespace

extern "C" int cl_frozen_rows(const cl_frozen_args* ap, void* stream) {
    if (ap == nullptr) return -1;
    const cl_frozen_args& a = *ap;
    const frozen_form f = frozen_form_of(a);
    if (int e = frozen_check(a, f)) return e;
    hipStream_t st = (hipStream_t)stream;
    // S = 1 (--mc-samples 1, the default) has its own instances; Laplace is an instance, Normal / Student-T a run-time kind (cl_math.h);
    // SUMS evaluates no likelihood and runs the run-time-kind instance whatever lik_kind says
    const bool one = a.S == 1, lap = a.lik_kind == CL_LIK_LAPLACE_ && f != frozen_form::SUMS;
    if (f == frozen_form::GROUPS) {
        if (lap) return one ? frozen_launch<frozen_laue_laplace_kernel<1>>(a, st) : frozen_launch<frozen_laue_laplace_kernel<8>>(a, st);
        return one ? frozen_launch<frozen_laue_kernel<1>>(a, st) : frozen_launch<frozen_laue_kernel<8>>(a, st);
    }
    const int e = lap ? (one ? frozen_launch<frozen_rows_laplace_kernel<1>>(a, st) : frozen_launch<frozen_rows_laplace_kernel<8>>(a, st))
                      : (one ? frozen_launch<frozen_rows_kernel<1>>(a, st) : frozen_launch<frozen_rows_kernel<8>>(a, st));
    if (e) return e;
    const long long t = ((a.n + 63) / 64) * a.S;
    return cl_launch<frozen_edges_kernel>(dim3((unsigned)((t + 255) / 256)), dim3(256), st, a);
}
