// What crosses compilation units below the C ABI (the argument structs are the public ones of include/careless_hip.h; every kernel file
// owns its extern "C" entry points: argument check, then launch), the one launch helper of the library, and the device helpers the
// kernel files share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstdio>
#include "../../include/careless_hip.h"

// What a scaler launch path hands down to the leaf that picks the kernel instance.  With a name sink the leaf prints the
// instance's own template parameters there and returns the length (cl_mlp_kernel_name: the name comes from the code that selects
// the instance) without touching the runtime; without one it launches on `grid` workgroups of stream `st`.
struct cl_launch_ctx {
    int grid;
    hipStream_t st;
    char* name = nullptr;
    size_t name_n = 0;
};

// A scaler launch: entry check, route, argument check, grid clamp, dispatch (mlp_launch.hip).  The units below it check nothing.
// `launch` false: the code the launch would return, without launching (cl_mlp_check).
int cl_launch_mlp(const cl_mlp_args* a, int mode, int grid, hipStream_t st, bool launch = true);
cl_route mlp_route(const cl_mlp_args& a, int mode);                                  // the unit or launcher cl_launch_mlp hands a launch to
cl_epilogue mlp_epilogue(const cl_mlp_args& a, int mode, cl_route r);                // the epilogue of the instance it runs (cl_mlp_epilogue)
struct MlpTraits { int K1; bool fixed_depth; };                                      // first-layer k-steps with real columns; depth compiled in
MlpTraits mlp_traits(const cl_mlp_args& a, int mode, cl_route r);                    // ... of the instance it runs (cl_mlp_instance_traits)
int cl_mlp_kernel_name_of(const cl_mlp_args& a, int mode, char* out, size_t n);     // the name of the instance the launch runs
// The seven compilations of elbo_mlp.hip (build.py), one cl_route each: -DCL_IMGL=0 CL_ROUTE_MLP, -DCL_IMGL=1 _IMGL (per-image layers),
// -DCL_IMGL=2 _PACKED (single-pass Laue), -DCL_CHAIN=1 _CHAIN (a block of a layer-block chain), -DCL_DET=1 _DET (deterministic mode: no
// atomics; plain layout, full step), -DCL_IMGL=2 -DCL_DET=1 _PACKED_DET, -DCL_CHAIN=1 -DCL_DET=1 _CHAIN_DET (a chain's LAST block: the
// forward-only and backward-only launches have no atomics and keep the chain unit).  One entry point, specialised in the unit of the route.
template <cl_route R>
int cl_mlp_unit(const cl_mlp_args& a, int mode, const cl_launch_ctx& c);
// The *_supports functions describe the shapes a kernel family holds; the A/B switches that keep shapes off a family are read by mlp_route only.
int cl_narrow_supports(const cl_mlp_args& a);                                       // elbo_narrow.hip: width <= 15, metadata <= 15, plain layout
int cl_launch_narrow(const cl_mlp_args& a, const cl_launch_ctx& c);                 // ... the full ELBO step on that kernel
int cl_lane_supports(const cl_mlp_args& a);                                         // elbo_lane.hip: lane = observation; 2 .. 20 layers, width <= 12, metadata <= 31 columns
#ifndef CL_LANE_WMAX
#define CL_LANE_WMAX 10                                                             // ... widest instance of every form (11, 12: twelve-wide, metadata in registers)
#endif
int cl_lane_imgl_supports(const cl_mlp_args& a);                                    // ... with one to three per-image layers on top
int cl_launch_lane_imgl(const cl_mlp_args& a, const cl_launch_ctx& c);
int cl_lane_block_supports(const cl_mlp_args& a, int mode);                          // ... a head-less layer block's forward / backward launch
int cl_launch_lane_block(const cl_mlp_args& a, int mode, const cl_launch_ctx& c);
int cl_launch_lane(const cl_mlp_args& a, const cl_launch_ctx& c);                   // ... the full ELBO step on that kernel
// elbo_step.hip: out[i] += the nparts partial rows of element i in index order (cl_reduce_partials; elbo_peel.hip and elbo_nlik.hip end in it)
int cl_launch_reduce_partials(const float* partials, int nparts, int P, float* out, const int* stop_flag, hipStream_t st);

// The likelihood of a launch, checked by every entry that evaluates one.  -1: a kind nobody compiles (it would run as Student-T), or
// Laplace beside an Evans-2011 buffer (cl_lik_ev11 has no Laplace form: the reference has no such class).  -2: Laplace at an entry whose
// kernels have no Laplace instance (`has_laplace` false: cl_wide_dense_forward_head_lik -- its caller then runs cl_slot_rows).  The lane
// and the narrow kernel have none either: cl_lane_*_supports / cl_narrow_supports answer 0 for the kind and mlp_route takes the launch to
// elbo_mlp.hip's instances (csrc/cl_math.h says why the kind is an instance and not a branch).
static inline int cl_lik_check(int lik_kind, const void* ev11, const void* d_ev11, const void* ev11_part, bool has_laplace) {
    if (lik_kind != CL_LIK_NORMAL_ && lik_kind != CL_LIK_STUDENTT_ && lik_kind != CL_LIK_LAPLACE_) return -1;
    if (lik_kind == CL_LIK_LAPLACE_ && (ev11 != nullptr || d_ev11 != nullptr || ev11_part != nullptr)) return -1;
    if (lik_kind == CL_LIK_LAPLACE_ && !has_laplace) return -2;
    return 0;
}

// Instantiated geometries of elbo_mlp.hip: the padded width WP fixes how many layers of activations + weight-gradient blocks fit in the
// 256-register budget of a wave: w <= 15 -> up to 20 layers (the CLI default scaler is 20 x 10), w <= 32 -> 10, w <= 64 -> 5.
// Per-image layers on more than 32 metadata columns at hidden width <= 15: the 16-wide instance <16, 64, 24, IMGL> (864 - 880 bytes of
// scratch per lane, the largest of the library) ends in a GPU memory fault when a workgroup walks more than one tile and crosses an
// image border (found by a random draw late in round 6: scripts/probe/imgl_abort_probe.py, NOTEBOOK R6.4; the forward-only launch
// is not affected).  Those shapes take the 32-wide instance, which holds up to CL_MLP_LMAX_W32 layers (deeper: the caller's
// layer-by-layer path, as for any scaler deeper than one launch).
// One helper for every unit's launch_mode and for mlp_route / mlp_epilogue (mlp_launch.hip); `imgl_unit`: the per-image-layer compilation
// (CL_IMGL == 1).  WP = 0: no instance holds the shape.
struct MlpGeom { int WP, DP, LMAX, KS; };
static inline MlpGeom mlp_geom(const cl_mlp_args& a, int mode, bool imgl_unit) {
    if (a.L < 1 || a.w < 1 || a.d < 1 || a.w > 64 || a.d > 64) return {0, 0, 0, 0};
    const int imgl = imgl_unit ? a.n_imgl : 0;
    const bool imgl_d64 = imgl_unit && mode != 1 && a.n_imgl > 0 && a.d > 32;
    MlpGeom g{0, a.d <= 8 ? 8 : (a.d <= 32 ? 32 : 64), 0, 4};
    if (a.w <= 15 && !imgl_d64) {
        // the narrow instance comes in three step counts (hidden width <= 8, <= 12, <= 15); the forward-only launch keeps all four
        g.WP = 16, g.LMAX = imgl_unit ? CL_MLP_LMAX_W16_IMGL : CL_MLP_LMAX_W16;
        if (mode != 1) g.KS = a.w <= 8 ? 2 : (a.w <= 12 ? 3 : 4);
    } else if (a.w == 16 && !imgl_unit) {
        g.WP = 16, g.LMAX = CL_MLP_LMAX_W16, g.KS = 5;         // (per-image layers keep the 32-wide instance)
    } else if (a.w <= 32) {
        g.WP = 32, g.LMAX = a.L + imgl <= 5 ? 5 : CL_MLP_LMAX_W32;
    } else {
        g.WP = 64, g.LMAX = CL_MLP_LMAX_W64;
    }
    if (a.L + imgl > g.LMAX) g.WP = 0;
    return g;
}
// The launches the plain epilogue is compiled for (template parameter EPI): a full step that draws its noise in the kernel keyed by the
// row itself, returns no predictions, has no Evans-2011 error model and at most two MC samples per epilogue lane.  Arguments only: which
// instances HAVE a plain epilogue (the 64-wide ones of the plain unit) and the A/B switch are mlp_epilogue's.
static inline cl_epilogue epi_plain(const cl_mlp_args& a, int mode) {
    if (mode != 0 || a.eta != nullptr || a.noise_row != nullptr || a.ipred_out != nullptr || a.S > 8) return CL_EPI_GENERIC;
    if (a.ev11 != nullptr || a.d_ev11 != nullptr || a.ev11_part != nullptr) return CL_EPI_GENERIC;
    if (a.lik_kind == CL_LIK_NORMAL_) return CL_EPI_PLAIN_NORMAL;
    return a.lik_kind == CL_LIK_STUDENTT_ ? CL_EPI_PLAIN_STUDENTT : CL_EPI_GENERIC;
}

// What the entry checks of wide_gemm.hip and elbo_frozen.hip ask of their required pointers.
template <class... P>
static inline bool any_null(const P*... p) { return ((p == nullptr) || ...); }

// THE launch of the library -- no other file holds a launch statement or reads the runtime's last error.  A kernel instance with `sm`
// bytes of dynamic LDS: -3 above the 160 KB of a gfx950 workgroup, else 0 or the hipError_t.  A call that issues several launches
// returns the first non-zero code and issues nothing behind it.
// The kernel is a template ARGUMENT, so the mark below -- the largest dynamic-LDS size the instance has been configured for -- is one
// per instance: the lane, narrow and 16/32/64-wide kernels share one function-pointer type, and a mark keyed by type would publish
// one instance's size for another.  One process drives one device; host threads may race here: setting the attribute twice is
// harmless, publishing a size that was not set is not, hence set first, then raise the mark.
template <auto Kern, class... A>
static inline int cl_launch_lds(dim3 grid, dim3 block, size_t sm, hipStream_t st, const A&... args) {
    if (sm > 160 * 1024) return -3;
    static std::atomic<size_t> configured{0};
    size_t have = configured.load(std::memory_order_acquire);
    if (have < sm) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
        if (e != hipSuccess) return (int)e;
        while (have < sm && !configured.compare_exchange_weak(have, sm, std::memory_order_release, std::memory_order_acquire)) {}
    }
    (void)hipGetLastError();   // drop any stale error of an unrelated earlier runtime call
    hipLaunchKernelGGL(Kern, grid, block, sm, st, args...);
    return (int)hipGetLastError();
}
// ... of a kernel without dynamic LDS
template <auto Kern, class... A>
static inline int cl_launch(dim3 grid, dim3 block, hipStream_t st, const A&... args) {
    return cl_launch_lds<Kern>(grid, block, 0, st, args...);
}

// ---------------------------------------------------------------------------------------------------------
// Device helpers the kernel files share (one copy of each)
// ---------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Full scheduling fence: pins the order of a hand-interleaved instruction stream, the scheduler may not move anything across it.
// Used to pin software-prefetched LDS operand reads ABOVE the MFMA group that runs while they are in flight: a wave issues in order
// and an MFMA issue blocks until the matrix pipe accepts it, so reads placed after a group of MFMAs only start when that group has
// drained; hipcc by itself keeps one operand buffer and emits exactly that order.
#define CL_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// Diagnostic build only (-DCL_STAMPS, `python -m careless_amd.build --stamps`, scripts/stamps*.py): per-wave cycle shares of the phases
// of a tile, accumulated in the kernel's st_acc[] / st_last.  The shipped library is built without it and executes no stamp.
#ifdef CL_STAMPS
#define STAMP(k)                                                                                   \
    do {                                                                                           \
        unsigned long long t_;                                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                 \
        st_acc[k] += t_ - st_last;                                                                 \
        st_last = t_;                                                                              \
    } while (0)
#define STAMP_VM(k)                                                                                \
    do {                                                                                           \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                           \
        STAMP(k);                                                                                  \
    } while (0)
#else
#define STAMP(k)
#define STAMP_VM(k)
#endif

// (wave-uniform base pointer) + (32-bit per-lane BYTE offset): the form hipcc lowers to `global_* v, v_off, s[base:base+1]`
// with no 64-bit per-lane address arithmetic (and nothing to keep live or spill across the tile loop)
template <class T>
__device__ __forceinline__ T ld_uo(const T* base, unsigned byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
template <class T>
__device__ __forceinline__ T* ptr_uo(T* base, unsigned byte_off) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off);
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// make a wave-uniform int opaque to loop-strength reduction (keeps per-tile base pointers in SGPRs, recomputed per tile)
__device__ __forceinline__ int opaque_uniform(int v) {
    v = __builtin_amdgcn_readfirstlane(v);
    asm volatile("" : "+s"(v));
    return v;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// LeakyReLU as max(x, leak x) with a bare v_max_f32: fmaxf() makes hipcc canonicalise x first (a second v_max per element) -- unless
// the unit is compiled with -fno-honor-nans, so A UNIT THAT CALLS THIS MUST BE BUILT WITH THAT FLAG (build.py: NNAN; every fused scaler
// unit is, since round 6).  Before that the bare instruction was inline assembly: opaque to hipcc's hazard recognizer, while its result
// is an MFMA operand of the next layer and gfx950 wants two wait states between a vector-ALU write and an MFMA reading it -- hipcc pads
// them only between instructions it knows (NOTEBOOK R6.1; scripts/check_lane_isa.py holds the library to the rule).  -DCL_LRELU_ASM
// rebuilds the old form.
__device__ __forceinline__ float lrelu(float x, float leak) {
    const float m = leak * x;
#ifdef CL_LRELU_ASM
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(m));
    return r;
#else
    return __builtin_fmaxf(x, m);
#endif
}
// dZ = dH * lrelu'(h): dH where h > 0, leak dH otherwise (h == 0 takes the leak branch, like `h > 0 ? ... : ...`; -0.0 cannot
// occur: h = max(x, leak x)).  A compare / conditional-move pair; the multiply + sign mask + bit select form the issue-time probe
// (scripts/probe/coissue_probe.hip) suggested was measured slower -- hipcc makes five instructions of it
// (scripts/patches/r2_narrow_closed_switches.diff, with the start stagger and the static priority of the second wave: no effect).
__device__ __forceinline__ float lrelu_bwd(float h, float dh, float leak) {
    return (h > 0.0f) ? dh : leak * dh;
}

// sum over the 64 lanes of a wave in double precision, left in every lane
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// block-wide double sum -> one atomic per block
__device__ __forceinline__ void block_atomic_add_d(double v, double* dst) {
    __shared__ double sh[16];
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
        atomicAdd(dst, s);
    }
}

// The kernel arguments, re-read from the kernarg segment behind an opaque pointer.  hipcc loads every field of a by-value argument
// struct at kernel entry and keeps it in SGPRs for the whole kernel (more than the ~100 there are: it then parks them in VGPR lanes
// and pays v_readlane / v_writelane in the per-tile code); fields that only one phase of a tile uses are loaded there instead, by
// scalar loads that cannot be hoisted.  Only valid in kernels whose single parameter is a `cl_mlp_args` by value.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) cl_mlp_args* cl_args_p;
__device__ __forceinline__ cl_args_p kernargs_again() {
    cl_args_p p = (cl_args_p)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// Cross-lane sums on the DPP network: no LDS round trip, one vector instruction per step (a __shfl_xor step is a ds_bpermute_b32
// plus its address arithmetic and an LDS latency in the middle of a dependent chain).
#define CL_DPP_ADD(x, ctrl, rmask) \
    ((x) + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (ctrl), (rmask), 0xF, false)))
// sum over each group of four consecutive lanes, left in all four
__device__ __forceinline__ float cl_quad_sum(float v) {
    v = CL_DPP_ADD(v, 0xB1, 0xF);   // quad_perm [1,0,3,2]
    v = CL_DPP_ADD(v, 0x4E, 0xF);   // quad_perm [2,3,0,1]
    return v;
}
// sum over each aligned group of S consecutive lanes (S = 1, 2, 4, 8 or 16: inside a 16-lane row), left in all lanes of the group
__device__ __forceinline__ float cl_group_sum(float v, int S) {
    if (S >= 2) v = CL_DPP_ADD(v, 0xB1, 0xF);
    if (S >= 4) v = CL_DPP_ADD(v, 0x4E, 0xF);
    if (S >= 8) v = CL_DPP_ADD(v, 0x141, 0xF);    // row_half_mirror
    if (S >= 16) v = CL_DPP_ADD(v, 0x140, 0xF);   // row_mirror
    return v;
}
// sum over the 64 lanes of a wave, returned as a wave-uniform value: a butterfly inside the 16-lane rows, then the rows through row_bcast
__device__ __forceinline__ float cl_wave_sum(float v) {
    v = cl_quad_sum(v);
    v = CL_DPP_ADD(v, 0x141, 0xF);  // row_half_mirror
    v = CL_DPP_ADD(v, 0x140, 0xF);  // row_mirror: every lane now holds its row's sum
    v = CL_DPP_ADD(v, 0x142, 0xA);  // row_bcast15 into rows 1 and 3
    v = CL_DPP_ADD(v, 0x143, 0xC);  // row_bcast31 into rows 2 and 3: lane 63 holds the total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// out[i] += sum over the `nparts` per-workgroup partials of element i, in index order (deterministic): the work of ONE 256-thread
// workgroup -- 32 consecutive elements x 8 chunks of the partial list; a thread sums its chunk (coalesced 128-B rows, eight rows in
// flight: a one-at-a-time loop is a chain of dependent HBM / MALL latencies), the 8 chunk sums are combined through LDS in chunk order.
// Shared by reduce_partials_kernel (elbo_step.hip) and the extra workgroups of the posterior backward kernels (elbo_q_kernels.h).
__device__ __forceinline__ void cl_reduce_partials_block(const float* __restrict__ partials, int nparts, int P, float* __restrict__ out, int block) {
    __shared__ float sh[8][33];
    const int e = threadIdx.x & 31, c = threadIdx.x >> 5;
    const int i = block * 32 + e;
    const int per = (nparts + 7) / 8;
    float s = 0.0f;
    if (i < P) {
        const int g1 = min(nparts, (c + 1) * per);
        int g = c * per;
        for (; g + 8 <= g1; g += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partials[(size_t)(g + k) * P + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; g < g1; ++g) s += partials[(size_t)g * P + i];
    }
    sh[c][e] = s;
    __syncthreads();
    if (c == 0 && i < P) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += sh[k][e];
        out[i] += t;
    }
}

// Image-scale gradients of a wave whose observations belong to MORE than one image (the rows of an image end inside the wave:
// stills with a few dozen reflections per image, or a reflection-owner shard that holds an eighth of every image's rows).  Image ids
// are sorted, so a wave holds a few images: one wave reduction and ONE atomic per image, image by image (up to four; a wave with more
// -- unsorted input -- finishes lane by lane).  `take`: this lane carries a term of a trainable image (img > 0); d_img[img - 1] += v.
__device__ __forceinline__ void cl_image_grad_segments(float* __restrict__ d_img, int img, float v, bool take, int lane) {
    unsigned long long m = __ballot(take);
    for (int it = 0; it < 4 && m != 0ull; ++it) {                      // wave-uniform
        const int first = __builtin_ctzll(m);
        const int im = __builtin_amdgcn_readlane(img, first);
        const bool mine = take && img == im;
        const float s = cl_wave_sum(mine ? v : 0.0f);
        if (lane == 0) atomicAdd(d_img + (im - 1), s);
        take = take && !mine;
        m = __ballot(take);
    }
    if (take) atomicAdd(d_img + (img - 1), v);
}
#else
typedef const cl_mlp_args* cl_args_p;                                        // (host pass over the kernel bodies: never executed)
__host__ __device__ inline cl_args_p kernargs_again() { return nullptr; }
__host__ __device__ inline float cl_quad_sum(float v) { return v; }
__host__ __device__ inline float cl_wave_sum(float v) { return v; }
__host__ __device__ inline float cl_group_sum(float v, int) { return v; }
__host__ __device__ inline void cl_image_grad_segments(float*, int, float, bool, int) {}
__host__ __device__ inline void cl_reduce_partials_block(const float*, int, int, float*, int) {}
#endif
