// nfk_step.h -- the integrator's elementwise arithmetic, shared by
// nfk_dynamics.hip (one trajectory per launch) and nfk_hmc_run.hip (all epochs
// of an HMC run per launch): ONE definition of the two update expressions, so a
// step inside either kernel has the same bits.  Include after
// <hip/hip_runtime.h>.
#ifndef NFK_STEP_H_
#define NFK_STEP_H_

#include <cstdint>

namespace {

// The integrator's constants: (float)dt, (float)dt_sq and the scheme.
struct Step {
    float dt, dt_sq;
    int path_len, verlet;
};

// x' = (x + v dt) + (G 0.5) dt_sq
__device__ __forceinline__ float step_x(float x, float v, float G, const Step& s) {
    return (x + v * s.dt) + (G * 0.5f) * s.dt_sq;
}

// v' = v + (dt (G + Gn)) 0.5
__device__ __forceinline__ float step_v(float v, float G, float Gn, const Step& s) {
    return v + (s.dt * (G + Gn)) * 0.5f;
}

inline Step make_step(int32_t path_len, double dt, double dt_sq, int32_t scheme) {
    // dt and dt**2 are the reference's Python scalars: rounded to fp32 once, where
    // the tensor op casts them
    Step s;
    s.dt = (float)dt;
    s.dt_sq = (float)dt_sq;
    s.path_len = path_len;
    s.verlet = scheme;
    return s;
}

}  // namespace

#endif  // NFK_STEP_H_
