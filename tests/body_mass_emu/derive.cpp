// TEST INFRASTRUCTURE ONLY -- host build of the routine that derives dof_invweight0, body_invweight0 and meaninertia from a sub-environment's body
// mass scale (gymnasium_amd/csrc/mjx_core.h derive_mass_constants, the body of mj_model_constants_kernel).  The device source is compiled with
// MJX_HOST_EMU, as tests/coop_emu does; one call is one lane: the scale row goes in through MassLaneFields::load_mass_scale with N = 1, the derived rows
// come out in the layout the kernel writes.  tests/test_body_mass_host.py compares them with compiler.scaled.  Nothing in the product links this file.
#define MJX_HOST_EMU 1
#include "../../gymnasium_amd/csrc/mjx_core.h"

namespace {
template <class M0>
int derive(const double *scale, double *out) {
    typedef mjx::MassLaneModel<M0> M;
    typedef mjx::MassLaneFields<M0> F;
    static double rows[F::WIDTH];
    for (int b = 0; b < M0::NBODY; b++) rows[F::OFF_MASS_SCALE + b] = scale[b];
    static F fields;
    fields.load_mass_scale(rows, 1, 0);
    static mjx::Data<M> d;
    d.bind(&fields);
    double dof[M0::NV], body[M0::NBODY][2], mean;
    mjx::derive_mass_constants<M>(d, dof, body, mean);
    int n = 0;
    for (int k = 0; k < M0::NV; k++) out[n++] = dof[k];
    for (int k = 0; k < 2 * M0::NBODY; k++) out[n++] = body[k / 2][k % 2];
    out[n++] = mean;
    return n;
}
}  // namespace

// model: the engine's MuJoCo kind order (half_cheetah, ant, humanoid, hopper, walker2d, inverted_pendulum, inverted_double_pendulum, reacher,
// humanoid_standup, swimmer, pusher); out: nv + 2 nbody + 1 doubles; returns that count, -1 for an unknown model
extern "C" __attribute__((visibility("default"))) int body_mass_derive(int model, const double *scale, double *out) {
    switch (model) {
    case 0: return derive<mjx::HalfCheetahModel>(scale, out);
    case 1: return derive<mjx::AntModel>(scale, out);
    case 2: return derive<mjx::HumanoidModel>(scale, out);
    case 3: return derive<mjx::HopperModel>(scale, out);
    case 4: return derive<mjx::Walker2dModel>(scale, out);
    case 5: return derive<mjx::InvertedPendulumModel>(scale, out);
    case 6: return derive<mjx::InvertedDoublePendulumModel>(scale, out);
    case 7: return derive<mjx::ReacherModel>(scale, out);
    case 8: return derive<mjx::HumanoidStandupModel>(scale, out);
    case 9: return derive<mjx::SwimmerModel>(scale, out);
    case 10: return derive<mjx::PusherModel>(scale, out);
    }
    return -1;
}
