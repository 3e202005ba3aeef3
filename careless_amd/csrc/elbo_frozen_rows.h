// The text of frozen_rows_kernel (csrc/elbo_frozen.hip), included there twice: as frozen_rows_kernel with the likelihood kind picked at run
// time (Normal / Student-T) and as frozen_rows_laplace_kernel with the Laplace likelihood compiled in.  Two expansions of one text rather than
// a template parameter or a shared body function: the run-time-kind kernel must stay what it was, instruction for instruction (a body
// function called from two kernels cost it five more spilled registers), under its old name.
//   #define CL_FROZEN_ROWS_KERNEL <name>     #define CL_FROZEN_ROWS_LAPLACE 0 | 1
template <int SB>
__global__ __launch_bounds__(FB) void CL_FROZEN_ROWS_KERNEL(const cl_frozen_args A) {
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

    // a row's seven numbers + the two reflection ids beside its wave, requested one chunk ahead: the chain row -> reflection -> amplitude is
    // two dependent loads deep and a thread has ~20 chunks to walk
    // `src` given (harmonic groups, second pass): the row's amplitude gradients were made by frozen_laue_kernel and wait in gbuf[src]: this
    // launch only sums them per reflection
    const bool gather = A.gbuf != nullptr;                 // (this kernel is only launched without gmeta: the second pass of harmonic groups)
    struct Row { int rid, rid_before, rid_after; float loc, sigma, io, sg, aim; long long key; };
    auto fetch = [&](long long c) -> Row {
        Row r;
        const long long row = c * FB + threadIdx.x, row0 = (row >> 6) << 6;
        const long long rc = row < n ? row : n - 1;
        r.rid = A.refl_id[rc];
        if (gather) {
            r.loc = r.sigma = r.io = 0.0f; r.sg = r.aim = 1.0f;
            r.key = A.src != nullptr ? (long long)A.src[rc] : rc;
        } else {
            r.loc = A.loc[rc]; r.sigma = A.sigma[rc]; r.io = A.iobs[rc]; r.sg = A.sig[rc];
            r.aim = A.aim != nullptr ? A.aim[rc] : 1.0f;
            r.key = A.key != nullptr ? (long long)A.key[rc] : A.obs_offset + row;
        }
        r.rid_before = (row0 > 0 && row0 <= n) ? A.refl_id[row0 - 1] : -1;
        r.rid_after = row0 + 64 < n ? A.refl_id[row0 + 64] : -1;
        return r;
    };
    Row nxt = fetch(blockIdx.x < chunks ? blockIdx.x : 0);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Row cur = nxt;
        if (c + gridDim.x < chunks) nxt = fetch(c + gridDim.x);
        const long long row = c * FB + threadIdx.x;
        const long long wv = row >> 6;                       // wave of the launch this row belongs to (edge record)
        const long long row0 = wv << 6;
        const bool in = row < n;
        int rid = cur.rid;
        if (!in) rid = -1;
        const bool act = rid >= 0;
        const float loc = cur.loc, sigma = cur.sigma, io = cur.io, sg = cur.sg, aim = cur.aim;
        const long long key = cur.key;
        // the runs of this wave: a lane adds the lane `off` above it while that lane belongs to the same reflection
        bool m[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int off = 1 << k;
            const int r2 = __shfl_down(rid, off);
            m[k] = (lane + off < 64) && r2 == rid;
        }
        const int prev = __shfl_up(rid, 1);
        const bool head = act && (lane == 0 || prev != rid);
        // ... and across the wave's two borders (wave-uniform)
        const int rid_first = __builtin_amdgcn_readlane(rid, 0), rid_last = __builtin_amdgcn_readlane(rid, 63);
        const int rid_before = cur.rid_before, rid_after = cur.rid_after;
        const bool first_cp = rid_first >= 0 && rid_first == rid_before;             // the first run continues the previous wave's last one
        const bool last_cn = rid_last >= 0 && rid_last == rid_after;                 // the last run continues in the next wave
        const bool single = rid_first == rid_last;
        const bool rec1 = last_cn && !(single && first_cp);                          // the last run STARTS here and goes on: head of a chain
        if (lane == 0 && row0 < n) {
            A.edge_rid[2 * wv] = first_cp ? (rid_first | ((single && last_cn) ? THROUGH : 0)) : -1;
            A.edge_rid[2 * wv + 1] = rec1 ? rid_last : -1;
        }
        // where this lane's run total goes (meaningful on head lanes): 0 dz_f, 1 edge record 0, 2 edge record 1
        const int route = (lane == 0 && first_cp) ? 1 : ((rid == rid_last && rec1) ? 2 : 0);
        const float inv_sg = cl_fast_rcp(sg), log_sg = cl_fast_log(sg);
        const float* __restrict__ eta_p = (A.eta != nullptr && !gather) ? A.eta + (size_t)(key - A.obs_offset) * S : nullptr;
        float* __restrict__ ip_p = (A.ipred_out != nullptr && !gather) ? A.ipred_out + (size_t)(key - A.obs_offset) * S : nullptr;
        const size_t zoff = (size_t)(act ? rid : 0) * S;

        for (int sb = 0; sb < S; sb += SB) {
            float e[SB], g[SB];
            if (gather) {
#pragma unroll
                for (int j = 0; j < SB; ++j) { e[j] = 0.0f; g[j] = (act && sb + j < S) ? A.gbuf[(size_t)key * S + sb + j] : 0.0f; }
            } else if (eta_p == nullptr) {
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
                if (gather) break;                                 // (wave-uniform)
                g[j] = 0.0f;
                if (sb + j < S && act) {                           // (the first test is wave-uniform)
                    const int s = sb + j;
                    const float zf = A.z_f[zoff + s];
                    const float tq = loc + sigma * e[j] + A.shift;
                    const float ipred = aim * tq * zf * zf;
                    if (ip_p != nullptr) ip_p[s] = ipred;
                    float dll, ll;
                    if (use_ev11) {
                        float gf, gb, ga;
                        ll = cl_lik_ev11(ipred, io, sg, A.lik_kind, A.dof, A.lik_const, ev, &dll, &gf, &gb, &ga);
                        g0 -= gf * A.w_ll; g1 -= ga * A.w_ll; g2 -= gb * A.w_ll;      // order: Sdfac, Sdadd, SdB
                    } else {
#if CL_FROZEN_ROWS_LAPLACE
                        ll = cl_lik_laplace_log_prob2(ipred, io, inv_sg, log_sg, &dll);
#else
                        ll = cl_lik_log_prob3(ipred, io, inv_sg, log_sg, A.lik_kind, A.dof, inv_dof, A.lik_const, &dll);
#endif
                    }
                    nll -= (double)ll * (double)A.w_ll;
                    g[j] = -dll * A.w_ll * aim * tq * 2.0f * zf;     // dNLL / d z_f[rid][s] of this row
                }
            }
            // run totals: suffix sums inside the runs, the first lane of a run ends with the run's total
#pragma unroll
            for (int k = 0; k < 6; ++k) {
#pragma unroll
                for (int j = 0; j < SB; ++j) {
                    if (sb + j < S) {
                        const float v = __shfl_down(g[j], 1 << k);
                        g[j] += m[k] ? v : 0.0f;
                    }
                }
            }
            if (head) {
#pragma unroll
                for (int j = 0; j < SB; ++j) {
                    if (sb + j < S) {
                        const int s = sb + j;
                        if (route == 0) {
                            if (A.accumulate) atomicAdd(A.dz_f + zoff + s, g[j]);
                            else A.dz_f[zoff + s] = g[j];
                        } else {
                            A.edge_val[(size_t)(2 * wv + (route - 1)) * S + s] = g[j];
                        }
                    }
                }
            }
        }
    }
    if (gather) return;                                        // (the first pass counted the NLL and the Evans-2011 terms)
    // NLL: one fp64 atomic per workgroup; Evans-2011 terms: one set per wave
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
