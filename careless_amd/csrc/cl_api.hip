// What libcareless_hip.so (include/careless_hip.h) answers without a kernel file of its own: the version, the binding handshake, the
// scaler's arithmetic queries and the thin scaler entries over cl_launch_mlp (mlp_launch.hip).  Every other extern "C" entry point sits
// in the file of its kernels -- argument check, then launch.
#include <hip/hip_runtime.h>
#include <cstring>
#include "cl_kernels.h"

extern "C" {

const char* cl_version(void) { return "careless_hip 0.1.0 (gfx950)"; }

// every argument struct of the header, by name
size_t cl_abi_sizeof(const char* struct_name) {
#define CL_ABI(T) {#T, sizeof(T)}
    static const struct { const char* name; size_t size; } table[] = {
        CL_ABI(cl_tn_args),     CL_ABI(cl_mlp_args),      CL_ABI(cl_adam_args), CL_ABI(cl_laue_args), CL_ABI(cl_det_args),
        CL_ABI(cl_frozen_args), CL_ABI(cl_refprior_args), CL_ABI(cl_rw_args),   CL_ABI(cl_nlik_args),
        CL_ABI(cl_sprior_args),
    };
#undef CL_ABI
    if (struct_name == nullptr) return 0;
    for (const auto& t : table)
        if (std::strcmp(t.name, struct_name) == 0) return t.size;
    return 0;
}

int cl_mlp_default_grid(void) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return cus;
}

int cl_mlp_max_layers(int w) {
    if (w < 1 || w > 64) return 0;
    return w <= 16 ? CL_MLP_LMAX_W16 : (w <= 32 ? CL_MLP_LMAX_W32 : CL_MLP_LMAX_W64);      // (width 16: the 16-wide instance with explicit biases, round 5)
}

int cl_mlp_meta_rows(int d) { return d < 1 ? 0 : ((d + 3) & ~3); }

size_t cl_mlp_param_count(int d, int w, int L) {
    if (d < 1 || w < 1 || L < 1) return 0;
    return (size_t)w * d + w + (size_t)(L - 1) * ((size_t)w * w + w) + 2 * (size_t)w + 2;
}

// the three scaler calls and the code they would return (mlp_launch.hip: entry check, route, argument check, launch)
int cl_elbo_mono_fwd_bwd(const cl_mlp_args* a, int grid, void* stream) { return cl_launch_mlp(a, 0, grid, (hipStream_t)stream); }
int cl_mlp_forward(const cl_mlp_args* a, int grid, void* stream) { return cl_launch_mlp(a, 1, grid, (hipStream_t)stream); }
int cl_mlp_backward_ext(const cl_mlp_args* a, int grid, void* stream) { return cl_launch_mlp(a, 2, grid, (hipStream_t)stream); }
int cl_mlp_check(const cl_mlp_args* a, int mode, int grid) { return cl_launch_mlp(a, mode, grid, nullptr, false); }

int cl_mlp_route(const cl_mlp_args* a, int mode) {
    if (a == nullptr || mode < 0 || mode > 2) return -1;
    return (int)mlp_route(*a, mode);
}

int cl_mlp_epilogue(const cl_mlp_args* a, int mode) {
    if (a == nullptr || mode < 0 || mode > 2) return -1;
    return (int)mlp_epilogue(*a, mode, mlp_route(*a, mode));
}

int cl_mlp_instance_traits(const cl_mlp_args* a, int mode) {
    if (a == nullptr || mode < 0 || mode > 2) return -1;
    const cl_route r = mlp_route(*a, mode);
    if (r == CL_ROUTE_NONE) return -2;
    const MlpTraits t = mlp_traits(*a, mode, r);
    return t.K1 | (t.fixed_depth ? CL_TRAIT_FIXED_DEPTH : 0);
}

int cl_mlp_kernel_name(const cl_mlp_args* a, int mode, char* out, size_t n) {
    if (a == nullptr || out == nullptr || n == 0 || mode < 0 || mode > 2) return -1;
    return cl_mlp_kernel_name_of(*a, mode, out, n);
}

}  // extern "C"
