// Host build of the Rice-Woolfson element math of careless_amd/csrc/cl_math.h for tests/test_rw_posterior.py (g++, no HIP):
// out[i] = {z, dz/dloc, dz/dscale, log q, dlog q/dz, dlog q/dloc, dlog q/dscale, y} of element i.
#include <cmath>
#include <cstdint>
#include "../careless_amd/csrc/cl_math.h"

extern "C" void rw_eval(int n, const float* a, const float* b, float eps, const unsigned char* centric, const float* n1, const float* n2, float* out) {
    for (int i = 0; i < n; ++i) {
        const cl_rw_elem t = cl_rw_sample(a[i], b[i], eps, centric[i] != 0, n1[i], n2[i]);
        float* o = out + 8 * (size_t)i;
        o[0] = t.z; o[1] = t.dz_dloc; o[2] = t.dz_dscale;
        o[3] = cl_rw_log_prob(t);
        cl_rw_log_prob_grads(t, o + 4, o + 5, o + 6);
        o[7] = t.y;
    }
}

// the normal pair of (seed, step, reflection idx, sample s), host forms of the transcendental pieces
extern "C" void rw_noise(unsigned long long seed, unsigned step, unsigned s, unsigned long long idx, float* n1, float* n2) {
    cl_noise_rw_pick(cl_noise_rw_block(seed, step, s, idx), s, n1, n2);
}
