// Host build of careless_amd/csrc/cl_math.h for tests/test_laplace.py: cl_lik_laplace_log_prob / cl_sign_bits per element, and the three
// two-way likelihood forms beside copies of the Normal / Student-T expressions as they stood before the Laplace kind existed (the two
// kinds must not move by a bit).
// Build:  g++ -O2 -shared -fPIC -o liblm.so laplace_math_check.cpp
#include "../careless_amd/csrc/cl_math.h"

// ---- the two-way forms of the parent ("Normal, else Student-T") ---------------------------------------------------------------------------
static float old_lik_log_prob(float ipred, float iobs, float sig, int kind, float dof, float lik_const, float* dll) {
    const float inv = 1.0f / sig;
    const float y = (ipred - iobs) * inv;
    if (kind == CL_LIK_NORMAL) {
        *dll = -y * inv;
        return -0.5f * y * y - 0.5f * CL_LOG_2PI_F - logf(sig);
    }
    const float y2 = y * y;
    *dll = -(dof + 1.0f) * y / (dof + y2) * inv;
    return -0.5f * (dof + 1.0f) * log1pf(y2 / dof) - logf(sig) + lik_const;
}
static float old_lik_log_prob2(float ipred, float iobs, float inv_sig, float log_sig, int kind, float dof, float lik_const, float* dll) {
    const float y = (ipred - iobs) * inv_sig;
    if (kind == CL_LIK_NORMAL) {
        *dll = -y * inv_sig;
        return -0.5f * y * y - 0.5f * CL_LOG_2PI_F - log_sig;
    }
    const float y2 = y * y;
    *dll = -(dof + 1.0f) * y / (dof + y2) * inv_sig;
    return -0.5f * (dof + 1.0f) * cl_log1p_pos(y2 / dof) - log_sig + lik_const;
}
static float old_lik_log_prob3(float ipred, float iobs, float inv_sig, float log_sig, int kind, float dof, float inv_dof, float lik_const,
                               float* dll) {
    const float y = (ipred - iobs) * inv_sig;
    if (kind == CL_LIK_NORMAL) {
        *dll = -y * inv_sig;
        return -0.5f * y * y - 0.5f * CL_LOG_2PI_F - log_sig;
    }
    const float y2 = y * y;
    const float den = dof + y2;
    float r = cl_fast_rcp(den);
    r = r * (2.0f - den * r);
    *dll = -(dof + 1.0f) * y * r * inv_sig;
    return -0.5f * (dof + 1.0f) * cl_log1p_pos(y2 * inv_dof) - log_sig + lik_const;
}

extern "C" {

// out[i][6] = (ll, dll) of cl_lik_log_prob, cl_lik_log_prob2, cl_lik_log_prob3; the hoisted forms get 1 / sig and logf(sig) as the kernels
// make them; old != 0: the parent's expressions
void lm_lik(int n, const float* ipred, const float* iobs, const float* sig, int kind, float dof, float lik_const, int old, float* out) {
    const float inv_dof = (kind == CL_LIK_STUDENTT) ? 1.0f / dof : 0.0f;
    for (int i = 0; i < n; ++i) {
        const float inv_sig = 1.0f / sig[i], log_sig = logf(sig[i]);
        float* o = out + 6 * i;
        if (old) {
            o[0] = old_lik_log_prob(ipred[i], iobs[i], sig[i], kind, dof, lik_const, o + 1);
            o[2] = old_lik_log_prob2(ipred[i], iobs[i], inv_sig, log_sig, kind, dof, lik_const, o + 3);
            o[4] = old_lik_log_prob3(ipred[i], iobs[i], inv_sig, log_sig, kind, dof, inv_dof, lik_const, o + 5);
        } else {
            o[0] = cl_lik_log_prob(ipred[i], iobs[i], sig[i], kind, dof, lik_const, o + 1);
            o[2] = cl_lik_log_prob2(ipred[i], iobs[i], inv_sig, log_sig, kind, dof, lik_const, o + 3);
            o[4] = cl_lik_log_prob3(ipred[i], iobs[i], inv_sig, log_sig, kind, dof, inv_dof, lik_const, o + 5);
        }
    }
}

void lm_sign(int n, const float* d, float* out) {
    for (int i = 0; i < n; ++i) out[i] = cl_sign_bits(d[i]);
}

// out[i][2] = (ll, dll) of cl_lik_laplace_log_prob
void lm_laplace(int n, const float* ipred, const float* iobs, const float* sig, float* out) {
    for (int i = 0; i < n; ++i) out[2 * i] = cl_lik_laplace_log_prob(ipred[i], iobs[i], sig[i], out + 2 * i + 1);
}

// ... of the hoisted form cl_lik_laplace_log_prob2, with 1 / sig and logf(sig) as the kernels make them
void lm_laplace2(int n, const float* ipred, const float* iobs, const float* sig, float* out) {
    for (int i = 0; i < n; ++i) out[2 * i] = cl_lik_laplace_log_prob2(ipred[i], iobs[i], 1.0f / sig[i], logf(sig[i]), out + 2 * i + 1);
}

int lm_kind_laplace(void) { return CL_LIK_LAPLACE; }

}  // extern "C"
