// TEST HARNESS (not product code): the two acceleration functors of the "rolled stages" step - AccelPinned (one tendon at a
// time) and AccelPaired (two in flight, gym_roboy_amd/csrc/msj_math.hpp) - compiled in ONE host translation unit, so that
// tests/test_accel_paired.py can hold them bit-equal: the pair form may change the order in which instructions are issued,
// never an expression or the order of the torque sums.
#include <string>
#include "../../gym_roboy_amd/csrc/msj_build.hpp"

// mode 0: qdd alone (both functors on the same state); mode 1 / 2: one env step, Euler / RK4 (step_rs against step_rs_paired).
// Outputs of the pinned form in (qa, va, fa), of the paired form in (qb, vb, fb); for mode 0 the accelerations are in qa / qb.
template <typename T>
static int run(const rb_robot_desc *d, double step_size, int nsub, int mode, long n, const T *q, const T *qd, const T *sp,
               T *qa, T *va, unsigned char *fa, T *qb, T *vb, unsigned char *fb) {
    using M = rb::MsjModel<T, 8>;
    std::string err;
    rb::MsjConst<T, 8> c;
    const int rc = rb::msj_build<T, 8>(d, step_size, nsub, &c, err);
    if (rc) return rc;
    for (long i = 0; i < n; ++i) {
        T u[8];
        for (int k = 0; k < 8; ++k) u[k] = M::prescale(c, k, sp[8 * i + k]);
        const rb::SpArray<T, 8> src{u};
        for (int j = 0; j < 3; ++j) { qa[3 * i + j] = qb[3 * i + j] = q[3 * i + j]; va[3 * i + j] = vb[3 * i + j] = qd[3 * i + j]; }
        if (mode == 0) {
            typename M::AccelPinned pinned{c, u};
            typename M::template AccelPaired<rb::SpArray<T, 8>> paired{c, src};
            pinned(q + 3 * i, qd + 3 * i, qa + 3 * i);
            paired(q + 3 * i, qd + 3 * i, qb + 3 * i);
            fa[i] = fb[i] = 1;
        } else if (mode == 1) {
            fa[i] = M::template step_rs<0>(c, qa + 3 * i, va + 3 * i, u);
            fb[i] = M::template step_rs_paired<0>(c, qb + 3 * i, vb + 3 * i, src);
        } else {
            fa[i] = M::template step_rs<1>(c, qa + 3 * i, va + 3 * i, u);
            fb[i] = M::template step_rs_paired<1>(c, qb + 3 * i, vb + 3 * i, src);
        }
    }
    return 0;
}
extern "C" int ap_run_f32(const rb_robot_desc *d, double step_size, int nsub, int mode, long n, const float *q, const float *qd,
                          const float *sp, float *qa, float *va, unsigned char *fa, float *qb, float *vb, unsigned char *fb) {
    return run<float>(d, step_size, nsub, mode, n, q, qd, sp, qa, va, fa, qb, vb, fb);
}
extern "C" int ap_run_f64(const rb_robot_desc *d, double step_size, int nsub, int mode, long n, const double *q, const double *qd,
                          const double *sp, double *qa, double *va, unsigned char *fa, double *qb, double *vb, unsigned char *fb) {
    return run<double>(d, step_size, nsub, mode, n, q, qd, sp, qa, va, fa, qb, vb, fb);
}
