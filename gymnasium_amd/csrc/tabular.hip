// tabular.hip -- the ToyText kernels as their own translation unit: namespace mi_tabular, the launch functions engine.hip calls for MI_ENV_TABULAR and
// MI_ENV_BLACKJACK once the arguments are validated and the buffers chosen (engine_types.h declares them), and every instantiation of the kernels of
// tabular_kernels.h.
//
// Why a unit, why the default flag set: which of the sixty-odd rollout forms runs -- table in LDS or not, general / branch-free / Blackjack kernel,
// with or without the extras -- is kernel selection, not ABI logic, and a change to it should not recompile the C ABI (nor the reverse).  Max-ILP
// scheduling cost these kernels 1 - 2 % (profiles/r04_maxilp_classic.txt), so they stay on the default scheduler, as they were in engine.o.
// The table itself is loaded by mi_tabular_load (engine.hip: host allocation).  No MuJoCo or classic-control code, and no part of the C ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "tabular_kernels.h"

namespace {
// f(std::true_type()) or f(std::false_type()): a run-time flag as a template argument of what f launches
template <class F>
void with_bool(bool flag, F &&f) {
    flag ? f(std::true_type()) : f(std::false_type());
}
}  // namespace

namespace mi_tabular {

int reset(mi_vecenv *v, const uint8_t *device_mask, int64_t *device_obs) {
    hipLaunchKernelGGL(tab_reset_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, device_mask, device_obs);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int step(mi_vecenv *v, const StepPtrs &p, double *info, double *final_info, bool fused_sample) {
    const TabStepPtrs tp = {(const int64_t *)p.actions, (int64_t *)p.obs, p.reward, p.terminated, p.truncated, (int64_t *)p.final_obs,
                            p.ep_ret, p.ep_len, info, final_info, p.act_lane, (int64_t *)p.actions_out, p.act_jump};
    const dim3 g(v->grid), b(kBlock);
    with_bool(fused_sample, [&](auto smp) {
        constexpr bool S = decltype(smp)::value;
        switch (v->cfg.autoreset_mode) {
        case MI_AUTORESET_NEXT_STEP: hipLaunchKernelGGL((tab_step_kernel<MI_AUTORESET_NEXT_STEP, S>), g, b, 0, v->stream, v->d, tp); break;
        case MI_AUTORESET_SAME_STEP: hipLaunchKernelGGL((tab_step_kernel<MI_AUTORESET_SAME_STEP, S>), g, b, 0, v->stream, v->d, tp); break;
        default: hipLaunchKernelGGL((tab_step_kernel<MI_AUTORESET_DISABLED, S>), g, b, 0, v->stream, v->d, tp); break;
        }
    });
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int rollout(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample, const RolloutExtra *ex) {
    const dim3 g(v->grid), b(kBlock);
    const TabTable &tab = v->d.tab;
    const bool next = v->cfg.autoreset_mode == MI_AUTORESET_NEXT_STEP;  // (mi_rollout refuses a DISABLED env)
    const bool full = p.actions_out && p.obs && p.reward && p.terminated && p.truncated;
    const int tk = tab.nS < 0 ? kTabBlackjack : (v->d.tab_fickle_rows ? kTabFickle : kTabPlain);
    static const bool lean_on = !(getenv("MI355ENV_TAB_LEAN") && getenv("MI355ENV_TAB_LEAN")[0] == '0');  // "0": tab_rollout_kernel (A/B, tests)
    // the branch-free kernels store no extras, draw their own actions and know NEXT_STEP only
    const bool lean = !ex && next && sample && lean_on;
    // ... for the collector's case: one plain table of <= 3 outcomes per (state, action) that fits into LDS in its packed form
    const int kl = tab.K == 1 ? 1 : 3;
    const size_t lean_lds = tk == kTabPlain && tab.nS > 0 ? (tab_lean_lds_bytes(tab.nS, tab.nA, kl) + 15) & ~(size_t)15 : 0;
    if (lean && tk == kTabPlain && !tab.env_table && tab.K <= 3 && lean_lds <= 150 * 1024) {
        const int nA = tab.nA, start = v->tab_start_state;
        const bool apow2 = nA >= 2 && (nA & (nA - 1)) == 0;
        int shift = 64;
        for (int x = nA; apow2 && x > 1; x >>= 1) shift--;
        with_bool(kl == 1, [&](auto k1) {
            with_bool(full, [&](auto full_c) {
                with_bool(start >= 0, [&](auto one_c) {
                    with_bool(apow2, [&](auto pow_c) {
                        hipLaunchKernelGGL((tab_rollout_lean_kernel<decltype(k1)::value ? 1 : 3, decltype(full_c)::value, decltype(one_c)::value, decltype(pow_c)::value>),
                                           g, b, lean_lds, v->stream, v->d, p, as, T, start, shift);
                    });
                });
            });
        });
    } else if (lean && tk == kTabBlackjack) {
        const char *fs = getenv("MI355ENV_BJ_FORCE_SLOW");  // tests: every k-th lane-step through the general routines
        const int force_slow = fs ? atoi(fs) : 0;
        with_bool(full, [&](auto full_c) {
            hipLaunchKernelGGL((bj_rollout_lean_kernel<decltype(full_c)::value>), g, b, 0, v->stream, v->d, p, as, T, force_slow);
        });
    } else {  // the general kernel, which also stores the extras
        // table in LDS when it fits next to the 160 KB of a CU and the copy is amortised over enough steps (Blackjack has no table)
        size_t lds = 0;
        if (tab.nS > 0 && T >= 8 && !tab.env_table) {  // (per-sub-environment tables stay in HBM / L2)
            const size_t cells = (size_t)tab.nS * tab.nA, rows = cells * tab.K;
            lds = (3 * rows + tab.nS) * sizeof(double) + (rows + cells) * sizeof(int32_t) + rows;
            lds = (lds + 15) & ~(size_t)15;
            if (lds > 150 * 1024) lds = 0;
        }
        const int lb = (int)lds;
        const RolloutExtra e = ex ? *ex : RolloutExtra{};
        with_bool(ex != nullptr, [&](auto with_extras) {
            with_bool(next, [&](auto next_c) {
                with_bool(sample, [&](auto smp) {
                    constexpr int M = decltype(next_c)::value ? MI_AUTORESET_NEXT_STEP : MI_AUTORESET_SAME_STEP;
                    constexpr bool S = decltype(smp)::value, X = decltype(with_extras)::value;
                    if (tk == kTabBlackjack)  // (no table)
                        hipLaunchKernelGGL((tab_rollout_kernel<M, S, false, kTabBlackjack, X>), g, b, 0, v->stream, v->d, p, as, T, lb, e);
                    else if (tk == kTabFickle && lds)
                        hipLaunchKernelGGL((tab_rollout_kernel<M, S, true, kTabFickle, X>), g, b, lds, v->stream, v->d, p, as, T, lb, e);
                    else if (tk == kTabFickle)
                        hipLaunchKernelGGL((tab_rollout_kernel<M, S, false, kTabFickle, X>), g, b, 0, v->stream, v->d, p, as, T, lb, e);
                    else if (lds)
                        hipLaunchKernelGGL((tab_rollout_kernel<M, S, true, kTabPlain, X>), g, b, lds, v->stream, v->d, p, as, T, lb, e);
                    else
                        hipLaunchKernelGGL((tab_rollout_kernel<M, S, false, kTabPlain, X>), g, b, 0, v->stream, v->d, p, as, T, lb, e);
                });
            });
        });
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace mi_tabular
