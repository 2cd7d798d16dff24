// Eigen-decomposition of a symmetric 3x3 matrix in registers (local_geometry.hip; the contract is pcc_local_geometry's,
// include/pcc_neighbour.h): a cyclic Jacobi iteration in float32 with the (0,1), (0,2), (1,2) rotations written out, a
// fixed number of sweeps, a three-element compare-exchange sort.  Every value is a named scalar: an array indexed at run
// time would live in scratch.  Host and device: the same arithmetic on either (the translation units are built with
// -ffp-contract=off), so the solver's accuracy can be measured without a GPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pcc {

constexpr int kJacobiSweeps = 4;  // a float32 model of the iteration converges in 4

// Eigenvalues ascending; (x_r, y_r, z_r) is the unit eigenvector of l_r.
struct Eigen3 {
    float l0, l1, l2;
    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
    float curv;
};

// One rotation in the (p, q) plane: annihilates a_pq.  r is the third axis, (v_ip, v_iq) the columns p and q of the
// accumulated rotations.  An off-diagonal entry that is exactly 0 is left alone, so an axis that is decoupled stays
// decoupled: its column stays a unit vector and its diagonal entry untouched.
__host__ __device__ __forceinline__ void jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p,
                                                       float &v0q, float &v1p, float &v1q, float &v2p, float &v2q) {
    if (apq == 0.f) return;
    // t = tan of the rotation angle, the smaller root: |t| <= 1.  (theta * theta may overflow to +inf: t = 0, a_pq is
    // then below the rounding of a_qq - a_pp.)
    const float theta = (aqq - app) / (apq + apq);
    const float tabs = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float t = theta < 0.f ? -tabs : tabs;
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c, h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.f;
    const float rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const float a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0;
    v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1;
    v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2;
    v2q = s * a2 + c * b2;
}

// (la, column a) and (lb, column b) in ascending order; equal values keep their places.
__host__ __device__ __forceinline__ void order_pair(float &la, float &lb, float &xa, float &ya, float &za, float &xb, float &yb,
                                                    float &zb) {
    if (la > lb) {
        float w;
        w = la, la = lb, lb = w;
        w = xa, xa = xb, xb = w;
        w = ya, ya = yb, yb = w;
        w = za, za = zb, zb = w;
    }
}

// The component of largest magnitude becomes non-negative (the lowest axis decides a tie); no -0.0 is left behind.
__host__ __device__ __forceinline__ void fix_sign(float &x, float &y, float &z) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const float lead = ax >= ay && ax >= az ? x : ay >= az ? y : z;
    if (lead < 0.f) x = -x, y = -y, z = -z;
    x = x + 0.f;
    y = y + 0.f;
    z = z + 0.f;
}

// The symmetric matrix (a00 a01 a02; . a11 a12; . . a22).
__host__ __device__ __forceinline__ Eigen3 sym3_eigen(float a00, float a01, float a02, float a11, float a12, float a22) {
    Eigen3 r;
    const float big = fmaxf(fmaxf(fmaxf(fabsf(a00), fabsf(a01)), fmaxf(fabsf(a02), fabsf(a11))), fmaxf(fabsf(a12), fabsf(a22)));
    // (fmaxf drops a NaN operand: test the sum as well)
    const float sum = ((((a00 + a01) + a02) + a11) + a12) + a22;
    if (!(big < INFINITY) || sum != sum) {
        const float nan = __builtin_bit_cast(float, 0x7fc00000u);
        r.l0 = r.l1 = r.l2 = r.curv = nan;
        r.x0 = r.y0 = r.z0 = r.x1 = r.y1 = r.z1 = r.x2 = r.y2 = r.z2 = nan;
        return r;
    }
    r.x0 = 1.f, r.y0 = 0.f, r.z0 = 0.f;
    r.x1 = 0.f, r.y1 = 1.f, r.z1 = 0.f;
    r.x2 = 0.f, r.y2 = 0.f, r.z2 = 1.f;
    if (big == 0.f) {
        r.l0 = r.l1 = r.l2 = r.curv = 0.f;
        return r;
    }
    // scaled by a power of two so that the largest entry is in [1/2, 1): exact, and clouds at any scale run the same
    // rotation arithmetic
    int e;
    (void)frexpf(big, &e);
    a00 = ldexpf(a00, -e), a01 = ldexpf(a01, -e), a02 = ldexpf(a02, -e);
    a11 = ldexpf(a11, -e), a12 = ldexpf(a12, -e), a22 = ldexpf(a22, -e);
    // (x_c, y_c, z_c) is column c of the accumulated rotations: the eigenvector of the diagonal entry c
#pragma unroll
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        jacobi_rotate(a00, a11, a01, a02, a12, r.x0, r.x1, r.y0, r.y1, r.z0, r.z1);
        jacobi_rotate(a00, a22, a02, a01, a12, r.x0, r.x2, r.y0, r.y2, r.z0, r.z2);
        jacobi_rotate(a11, a22, a12, a01, a02, r.x1, r.x2, r.y1, r.y2, r.z1, r.z2);
    }
    order_pair(a00, a11, r.x0, r.y0, r.z0, r.x1, r.y1, r.z1);
    order_pair(a11, a22, r.x1, r.y1, r.z1, r.x2, r.y2, r.z2);
    order_pair(a00, a11, r.x0, r.y0, r.z0, r.x1, r.y1, r.z1);
    fix_sign(r.x0, r.y0, r.z0);
    fix_sign(r.x1, r.y1, r.z1);
    fix_sign(r.x2, r.y2, r.z2);
    const float trace = (a00 + a11) + a22;
    r.curv = trace > 0.f ? fmaxf(a00, 0.f) / trace : 0.f;
    r.l0 = ldexpf(a00, e), r.l1 = ldexpf(a11, e), r.l2 = ldexpf(a22, e);
    return r;
}

}  // namespace pcc
