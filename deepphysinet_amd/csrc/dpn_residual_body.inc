// The residual body of dpn_residual_kernel / dpn_residual_points_kernel (dpn_residual.hip) and dpn_causal_bins_kernel (dpn_causal.hip), included by each:
// inverse_norm (+ clip), the chained Jacobian J, and the six signed residuals r[e] = lhs - rhs of interface_physics.py:97-185 at point `ic` of
// the kernel argument `a` (out_n, jac_n, f, ph).  Leaves val, msk, J, the named fields, omega, delta, Fv, K and r in scope.
    constexpr float C_P = 1005.f, L_V = 2.5e6f, R_V = 461.5f, R_D = 287.f, EPS = 1e-6f;
    float val[6], msk[6], J[6][3];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float v = a.out_n[ic * 6 + k] * a.ph.std[k] + a.ph.mean[k];       // inverse_norm (interface_physics.py:250)
        float dv = a.ph.std[k];                                          // d val / d out
        if (a.ph.sq_on[k]) { dv = 2.f * v * a.ph.std[k]; v = v * v + a.ph.sq_add[k]; }   // three-factor min_max: squared, shifted (:244-247)
        float m = 1.f;
        if (a.ph.clip_on[k]) {                                           // torch.clip: gradient passes where lo <= v <= hi
            m = (v >= a.ph.clip_lo[k] && v <= a.ph.clip_hi[k]) ? 1.f : 0.f;
            v = fminf(fmaxf(v, a.ph.clip_lo[k]), a.ph.clip_hi[k]);
        }
        val[k] = v; msk[k] = m * dv;
#pragma unroll
        for (int c = 0; c < 3; ++c) J[k][c] = a.jac_n[(ic * 6 + k) * 3 + c] * msk[k];
    }
    const float u = val[0], v = val[1], p = val[2], T = val[3], q = val[4], rho = val[5];
    const float fc = a.f[ic];
    const float omega = J[2][2] + u * J[2][0] + v * J[2][1];
    const float A = J[3][2] + u * J[3][0] + v * J[3][1];
    const float B = J[4][2] + u * J[4][0] + v * J[4][1];
    const float tc = T - 273.15f;
    const float e_s = 6.112f * expf(17.67f * tc / (tc + 243.5f)) * 100.f;                 // get_qs :181-185
    const float qs_raw = 0.622f * e_s / (p - 0.378f * e_s);
    const float q_s = (qs_raw != qs_raw) ? qs_raw : fmaxf(qs_raw, 1e-6f);          // torch.maximum propagates NaN (:166)
    const float delta = (omega < 0.f && q >= q_s) ? 1.f : 0.f;
    const float R = (1.f + 0.608f * q) * R_D;
    const float Fv = (L_V * R - C_P * R_V * T) / (C_P * R_V + T * T + L_V * L_V * q_s) * q_s * T;   // precedence as written :161-163
    const float K = delta * Fv / (p + EPS);
    float r[6];
    r[0] = J[0][2] + u * J[0][0] + v * J[0][1] + J[2][0] / rho - fc * v;                   // :97-104
    r[1] = J[1][2] + u * J[1][0] + v * J[1][1] + J[2][1] / rho + fc * u;                   // :106-114
    r[2] = J[5][2] + u * J[5][0] + v * J[5][1] + rho * J[0][0] + rho * J[1][1];            // :116-124
    r[3] = C_P * A - omega / (rho + EPS) + L_V * B;                                        // :126-144
    r[4] = -omega * K + B;                                                                 // :146-175
    r[5] = p - rho * (1.f + 0.608f * q) * R_D * T;                                         // :177-179
