// plane_update_xform.inc -- step 1 of MapPlane::UpdateCoefficientsAndPoints(Frame, id) (reference src/MapPlane.cc:337-341): the matrix
// handed to pcl::transformPointCloud is Converter::toSE3Quat(pF.mTcw) -> Eigen::Isometry3d -> inverse().  Host arithmetic in double; plain
// C++ without headers of its own so that a stand-alone host program can include it (tools/plane_update_host.cpp).  Compile with
// -ffp-contract=off: none of the sums below may be contracted.
//
//   R, t           the float entries of Tcw widened to double (Converter.cc:46-59)
//   q              Eigen::Quaterniond(R): the trace branch, else the largest diagonal entry (QuaternionBase::operator=(Matrix))
//   SE3Quat(R, t)  w < 0 flips the sign, then q /= sqrt(w w + x x + y y + z z) (se3quat.h:66-73, normalizeRotation)
//   Isometry3d     q.toRotationMatrix() and t
//   inverse()      Isometry mode: L = R'^T, translation (-L) t, each three-term sum left to right
// The readings of Quaterniond(Matrix3d) and toRotationMatrix are the ones tests/pose_opt_ref.py states (DESIGN.md, pose optimisation readings (1)).
// M: rows 0..2 of the 4 x 4 matrix, row-major 3 x 4.
static inline void hvo_pu_transform(const float Tcw[12], double M[12])
{
    double m[3][3], t[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) m[r][c] = (double)Tcw[4 * r + c]; t[r] = (double)Tcw[4 * r + 3]; }
    double q[4] = { 0.0, 0.0, 0.0, 0.0 };                        // w, x, y, z
    double tr = m[0][0] + m[1][1] + m[2][2];
    if (tr > 0.0) {
        tr = __builtin_sqrt(tr + 1.0); q[0] = 0.5 * tr; tr = 0.5 / tr;
        q[1] = (m[2][1] - m[1][2]) * tr; q[2] = (m[0][2] - m[2][0]) * tr; q[3] = (m[1][0] - m[0][1]) * tr;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        tr = __builtin_sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0); q[1 + i] = 0.5 * tr; tr = 0.5 / tr;
        q[0] = (m[k][j] - m[j][k]) * tr; q[1 + j] = (m[j][i] + m[i][j]) * tr; q[1 + k] = (m[k][i] + m[i][k]) * tr;
    }
    if (q[0] < 0.0) for (int c = 0; c < 4; c++) q[c] = -q[c];
    const double nrm = __builtin_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[3][3] = { { 1 - (tyy + tzz), txy - twz, txz + twy }, { txy + twz, 1 - (txx + tzz), tyz - twx }, { txz - twy, tyz + twx, 1 - (txx + tyy) } };
    for (int r = 0; r < 3; r++) {
        const double l0 = R[0][r], l1 = R[1][r], l2 = R[2][r];
        M[4 * r] = l0; M[4 * r + 1] = l1; M[4 * r + 2] = l2;
        M[4 * r + 3] = ((-l0) * t[0] + (-l1) * t[1]) + (-l2) * t[2];
    }
}
