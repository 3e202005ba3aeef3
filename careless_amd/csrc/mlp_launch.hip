// The launch layer of the scaler kernels (host code only, no kernel): every cl_elbo_mono_fwd_bwd / cl_mlp_forward / cl_mlp_backward_ext
// call is decided here -- entry check, mlp_route, mlp_check, grid clamp, mlp_dispatch -- and handed to the lane kernel's launch layer
// (elbo_lane.hip), the narrow kernel (elbo_narrow.hip) or the unit of elbo_mlp.hip that compiles the route (cl_mlp_unit<route>).
// cl_mlp_route, cl_mlp_epilogue, cl_mlp_instance_traits, cl_mlp_check and cl_mlp_kernel_name answer from the same functions without launching.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "cl_kernels.h"

// The A/B switches (bisection and measurement runs; unset or anything but "0" = on), read here and nowhere else.  Each keeps shapes off
// a kernel family, which then go to the next kernel down mlp_route's order:
//   CARELESS_HIP_LANE=0         every shape off the lane-per-observation kernel (elbo_lane.hip)
//   CARELESS_HIP_NARROW=0       every shape off elbo_narrow.hip
//   CARELESS_HIP_LANE_W12=0     widths 11, 12 off the lane kernel (the narrow kernel they ran on until round 6)
//   CARELESS_HIP_LANE_DEPTHS=0  depths other than the default off the lane kernel (until round 5)
//   CARELESS_HIP_LANE_BLOCKS=0  the head-less blocks of a chain off the lane kernel (the chain unit of elbo_mlp.hip)
// and two keep launches off an instance of the kernel the route names:
//   CARELESS_HIP_EPI=0          the 64-wide instances off their plain epilogue (the generic one: every launch until this switch came)
//   CARELESS_HIP_EXACT=0        the plain-epilogue instances off their exact forms (mlp_traits): all DP / 4 metadata k-steps and the
//                               run-time depth, every launch's instance until this switch came.  Measurement only, for telling the two apart:
//                               exactly "k1" keeps the trimmed k-steps alone, exactly "depth" the compile-time depth alone
struct RouteSwitches { bool lane, narrow, w12, depths, blocks, epi, exact_k1, exact_depth; };
static bool switch_on(const char* name) { const char* e = getenv(name); return !(e != nullptr && e[0] == '0'); }
// (one part of a two-part switch: off with the switch, and when the value is exactly the OTHER part's word -- measurement runs only)
static bool switch_part(const char* name, const char* other) { const char* e = getenv(name); return switch_on(name) && !(e != nullptr && strcmp(e, other) == 0); }
static const RouteSwitches& route_switches() {
    static const RouteSwitches s{switch_on("CARELESS_HIP_LANE"), switch_on("CARELESS_HIP_NARROW"), switch_on("CARELESS_HIP_LANE_W12"),
                                 switch_on("CARELESS_HIP_LANE_DEPTHS"), switch_on("CARELESS_HIP_LANE_BLOCKS"), switch_on("CARELESS_HIP_EPI"),
                                 switch_part("CARELESS_HIP_EXACT", "depth"), switch_part("CARELESS_HIP_EXACT", "k1")};
    return s;
}
// The epilogue of the instance a launch on route `r` runs (cl_mlp_epilogue; the plain unit's launch_mode picks the instance by it).
cl_epilogue mlp_epilogue(const cl_mlp_args& a, int mode, cl_route r) {
    if (r != CL_ROUTE_MLP || !route_switches().epi || mlp_geom(a, mode, false).WP != 64) return CL_EPI_GENERIC;
    return epi_plain(a, mode);
}
// What the instance a launch on route `r` runs is compiled for beyond its printed name (cl_mlp_instance_traits; the plain unit's
// launch_plain64 picks the instance by it).  The plain-epilogue 64-wide instances come in exact forms: on 32 padded metadata columns
// with the 6 k-steps that 8 < d <= 24 real columns fill, and on up to 32 with the depth compiled in when the launch runs all LMAX layers.
MlpTraits mlp_traits(const cl_mlp_args& a, int mode, cl_route r) {
    if (r < CL_ROUTE_MLP) return {0, false};                             // (the lane and narrow kernels: no MFMA k-steps of this kind)
    const MlpGeom g = mlp_geom(a, mode, r == CL_ROUTE_MLP_IMGL);
    MlpTraits t{g.DP / 4, false};
    if (mlp_epilogue(a, mode, r) == CL_EPI_GENERIC) return t;
    const RouteSwitches& sw = route_switches();
    if (sw.exact_k1 && g.DP == 32 && a.d <= 24) t.K1 = 6;
    if (sw.exact_depth && g.DP <= 32 && a.L == g.LMAX) t.fixed_depth = true;
    return t;
}

// Which launcher takes the launch: the one routing decision of the scaler launches (cl_launch_mlp, cl_mlp_kernel_name_of, cl_mlp_route).
// Shape, optional buffers and mode only: n_pad, the grid and the buffers a route requires are mlp_check's.
cl_route mlp_route(const cl_mlp_args& a, int mode) {
    const RouteSwitches& sw = route_switches();
    const bool lane_depth = sw.depths || a.L == CL_MLP_LMAX_W16;
    const bool lane = mode == 0 && sw.lane && lane_depth && (sw.w12 || a.w <= CL_LANE_WMAX) && cl_lane_supports(a);
    const bool narrow = mode == 0 && sw.narrow && cl_narrow_supports(a);
    const bool lane_imgl = mode == 0 && a.n_imgl > 0 && sw.lane && lane_depth && cl_lane_imgl_supports(a);
    cl_route r;
    if (a.dzf_obs != nullptr && (mode == 0 || (a.act_out == nullptr && a.dH_ext == nullptr))) {
        // deterministic mode: full steps only, with the Evans-2011 gradients in their per-wave slots.  The default scaler's shapes keep their
        // own kernels (round 4: elbo_lane.hip / elbo_narrow.hip store per observation when dzf_obs is given), per-image layers the lane
        // kernel's instances only (round 6: one wave per image; the IMGL instances of elbo_mlp.hip keep their float atomics), every other width
        // <= 64 runs the deterministic compilations of elbo_mlp.hip.  (The forward-only and backward-only launches of a layer-block chain have
        // no float atomics: they take the chain unit.)
        if (mode != 0 || (a.ev11 != nullptr && a.ev11_part == nullptr)) return CL_ROUTE_NONE;
        if (a.n_imgl > 0) r = lane_imgl ? CL_ROUTE_LANE_IMGL : CL_ROUTE_NONE;
        else if (a.dX_out != nullptr) r = (a.row_map != nullptr || a.act_out != nullptr || a.dH_ext != nullptr) ? CL_ROUTE_NONE : CL_ROUTE_MLP_CHAIN_DET;
        else if (lane) r = CL_ROUTE_LANE;
        else if (narrow) r = CL_ROUTE_NARROW;
        else if (a.row_map != nullptr && a.n_imgl == 0) r = CL_ROUTE_MLP_PACKED_DET;            // single-pass Laue, wider than 15
        else r = (a.row_map != nullptr || a.act_out != nullptr || a.dH_ext != nullptr) ? CL_ROUTE_NONE : CL_ROUTE_MLP_DET;
    } else if ((a.act_out != nullptr || a.dH_ext != nullptr) && sw.lane && sw.blocks && cl_lane_block_supports(a, mode)) {
        r = CL_ROUTE_LANE_BLOCK;              // the first block of a chained narrow scaler: the lane kernel's forward-only / external-gradient instances (round 6)
    } else if (a.act_out != nullptr || a.dH_ext != nullptr || a.dX_out != nullptr) {
        r = (a.row_map != nullptr || a.n_imgl > 0) ? CL_ROUTE_NONE : CL_ROUTE_MLP_CHAIN;        // (chains use the plain layout)
    } else if (a.n_imgl > 0) {
        r = lane_imgl ? CL_ROUTE_LANE_IMGL : CL_ROUTE_MLP_IMGL;       // packed layout + per-image layers: the default scaler's shapes on the lane kernel (round 5)
    } else if (lane) {
        r = CL_ROUTE_LANE;                    // the default scaler's shape: lane = observation
    } else if (narrow) {
        r = CL_ROUTE_NARROW;                  // hidden width <= 15: one wave per SIMD
    } else {
        r = a.row_map != nullptr ? CL_ROUTE_MLP_PACKED : CL_ROUTE_MLP;
    }
    // dZ0_out (the launch behind a peeled first layer, elbo_peel.hip) is stored by the default scaler's kernels only: a launch elsewhere
    // would ignore it and leave the peeled layer a zero gradient without any error
    if (a.dZ0_out != nullptr && r != CL_ROUTE_LANE && r != CL_ROUTE_NARROW && r != CL_ROUTE_LANE_IMGL) return CL_ROUTE_NONE;
    if (r >= CL_ROUTE_MLP && mlp_geom(a, mode, r == CL_ROUTE_MLP_IMGL).WP == 0) return CL_ROUTE_NONE;     // wider / deeper than elbo_mlp.hip's instances
    return r;
}

// Every argument check of a scaler launch, in one place: mlp_entry is what the call of a mode (0 = cl_elbo_mono_fwd_bwd, 1 =
// cl_mlp_forward, 2 = cl_mlp_backward_ext) asks before anything else, mlp_check what cl_launch_mlp tests between the route and the
// dispatch.  Precedence: the entry's -1 (the likelihood: cl_lik_check), then -1 tile / grid, -2 no route, the route's own -1 clauses, the -4 bounds.
static int mlp_entry(const cl_mlp_args* a, int mode) {
    if (a == nullptr || a->meta_t == nullptr || a->mlp == nullptr) return -1;
    if (a->n_obs <= 0 || a->n_pad < a->n_obs || a->n_pad % CL_MLP_TILE != 0) return -1;
    switch (mode) {
        case 0:
            if (a->refl_id == nullptr || a->iobs == nullptr || a->sig == nullptr || a->z_f == nullptr || a->dz_f == nullptr ||
                a->partials == nullptr || a->scalars == nullptr || a->S < 1 || a->R < 1)
                return -1;
            if (a->use_img && (a->image_id == nullptr || a->img == nullptr || a->d_img == nullptr)) return -1;
            return cl_lik_check(a->lik_kind, a->ev11, a->d_ev11, a->ev11_part, true);
        case 1: return (a->act_out == nullptr && (a->loc_out == nullptr || a->sig_out == nullptr)) ? -1 : 0;
        case 2: return ((a->dO_ext == nullptr && a->dH_ext == nullptr) || a->partials == nullptr) ? -1 : 0;
    }
    return -1;
}
// The kernels address with 32-bit byte offsets: a float array of `elems` elements must stay below 4 GiB (shard further across GPUs otherwise).
static inline bool over_4gib(unsigned long long elems) { return 4ull * elems >= (1ull << 32); }
static inline bool meta_over(const cl_mlp_args& a) { return over_4gib((unsigned long long)((a.d + 3) & ~3) * (unsigned long long)a.n_pad); }   // meta_t
static inline bool refl_over(const cl_mlp_args& a) { return over_4gib((unsigned long long)a.R * (unsigned long long)a.S); }                     // z_f, dz_f
static inline bool obs_over(const cl_mlp_args& a) { return over_4gib((unsigned long long)a.n_pad * (unsigned long long)a.S); }                  // eta, ipred_out, dzf_obs

static int mlp_check(const cl_mlp_args& a, int mode, int grid, cl_route r) {
    if (a.n_pad % CL_MLP_TILE != 0 || a.n_pad <= 0 || grid < 1) return -1;
    if (r == CL_ROUTE_NONE) return -2;
    const bool packed = a.row_map != nullptr || r == CL_ROUTE_MLP_IMGL;      // (the route keeps row_map off the plain-layout launchers)
    // deterministic mode: the routes with per-observation stores (the lane and narrow kernels store when dzf_obs is given)
    const bool det = r == CL_ROUTE_MLP_DET || r == CL_ROUTE_MLP_PACKED_DET || r == CL_ROUTE_MLP_CHAIN_DET ||
                     (a.dzf_obs != nullptr && (r == CL_ROUTE_LANE || r == CL_ROUTE_LANE_IMGL || r == CL_ROUTE_NARROW));
    if (r == CL_ROUTE_MLP_PACKED_DET && a.n_obs != a.n_pad) return -2;      // (this unit's answer to a padded packed layout has always been -2)
    if (packed) {                                                           // packed layout: no padding rows behind n_obs, group sizes with their tile maxima, full step only
        if (a.row_map == nullptr || a.n_obs != a.n_pad || a.n_imgl < 0) return -1;
        if (a.gmeta != nullptr && (a.tile_gmax == nullptr || mode != 0)) return -1;
    }
    if (r == CL_ROUTE_MLP_IMGL) {                                           // per-image layers: their weights, the tiles' images, and no image scale beside them
        if (a.imgl == nullptr || a.tile_img == nullptr || a.n_images < 1 || a.use_img) return -1;
        if (mode != 1 && a.d_imgl == nullptr) return -1;
    }
    if (r == CL_ROUTE_MLP_CHAIN) {                                          // a block's activations leave the forward launch, its gradient enters the backward one
        if (a.act_out != nullptr && mode != 1) return -1;
        if (a.dH_ext != nullptr && mode != 2) return -1;
    }
    if (det && (a.nll_part == nullptr || (a.use_img && a.dimg_obs == nullptr))) return -1;      // the store targets
    if (meta_over(a)) return -4;
    if (r != CL_ROUTE_LANE_BLOCK && refl_over(a)) return -4;                 // (a head-less block reads no reflection)
    if ((det || (packed && (a.eta != nullptr || a.ipred_out != nullptr))) && obs_over(a)) return -4;
    return 0;
}

// The launcher or unit the route names: every one takes the launch through `c`, and with a name sink there (cl_mlp_kernel_name_of) the
// leaf that picks the instance prints it.
static int mlp_dispatch(const cl_mlp_args& a, int mode, cl_route r, const cl_launch_ctx& c) {
    switch (r) {
        case CL_ROUTE_NONE: break;
        case CL_ROUTE_LANE: return cl_launch_lane(a, c);
        case CL_ROUTE_LANE_IMGL: return cl_launch_lane_imgl(a, c);
        case CL_ROUTE_LANE_BLOCK: return cl_launch_lane_block(a, mode, c);
        case CL_ROUTE_NARROW: return cl_launch_narrow(a, c);
        case CL_ROUTE_MLP: return cl_mlp_unit<CL_ROUTE_MLP>(a, mode, c);
        case CL_ROUTE_MLP_PACKED: return cl_mlp_unit<CL_ROUTE_MLP_PACKED>(a, mode, c);
        case CL_ROUTE_MLP_IMGL: return cl_mlp_unit<CL_ROUTE_MLP_IMGL>(a, mode, c);
        case CL_ROUTE_MLP_CHAIN: return cl_mlp_unit<CL_ROUTE_MLP_CHAIN>(a, mode, c);
        case CL_ROUTE_MLP_DET: return cl_mlp_unit<CL_ROUTE_MLP_DET>(a, mode, c);
        case CL_ROUTE_MLP_PACKED_DET: return cl_mlp_unit<CL_ROUTE_MLP_PACKED_DET>(a, mode, c);
        case CL_ROUTE_MLP_CHAIN_DET: return cl_mlp_unit<CL_ROUTE_MLP_CHAIN_DET>(a, mode, c);
    }
    return -2;
}

int cl_launch_mlp(const cl_mlp_args* ap, int mode, int grid, hipStream_t st, bool launch) {
    if (int e = mlp_entry(ap, mode)) return e;
    const cl_mlp_args& a = *ap;
    const cl_route r = mlp_route(a, mode);
    if (int e = mlp_check(a, mode, grid, r)) return e;
    if (!launch) return 0;
    if (grid > a.n_pad / CL_MLP_TILE) grid = a.n_pad / CL_MLP_TILE;
    return mlp_dispatch(a, mode, r, {grid, st});
}

// Name of the kernel instance cl_launch_mlp(a, mode, ...) runs (bench.py and the profiling scripts label their rows with it instead of
// guessing): for shapes, not for valid buffers -- the same dispatch without the checks, with a name sink for the leaf that picks the
// instance.  Returns the length written (snprintf semantics).
int cl_mlp_kernel_name_of(const cl_mlp_args& a, int mode, char* out, size_t n) {
    const cl_route r = mlp_route(a, mode);
    if (r == CL_ROUTE_NONE) return snprintf(out, n, "(unsupported)");
    return mlp_dispatch(a, mode, r, {0, nullptr, out, n});
}
