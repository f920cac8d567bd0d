// kinhip_m34.h -- rigid transforms of the host staging code (fp64).
#pragma once
#include <cmath>
#include <cstring>

namespace kinhip {

// rigid 3x4, row-major rotation
struct M34 {
    double r[9];
    double t[3];
};

inline M34 m_identity() {
    M34 m{};
    m.r[0] = m.r[4] = m.r[8] = 1.0;
    return m;
}

inline bool m_is_identity(const M34& m) {
    const M34 I = m_identity();
    return memcmp(&m, &I, sizeof(M34)) == 0;
}

inline M34 m_mul(const M34& a, const M34& b) {
    M34 c;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            c.r[3 * i + j] = a.r[3 * i] * b.r[j] + a.r[3 * i + 1] * b.r[3 + j] + a.r[3 * i + 2] * b.r[6 + j];
        c.t[i] = a.r[3 * i] * b.t[0] + a.r[3 * i + 1] * b.t[1] + a.r[3 * i + 2] * b.t[2] + a.t[i];
    }
    return c;
}

inline M34 m_from_col16(const double* T) {
    M34 m;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m.r[3 * i + j] = T[i + 4 * j];
        m.t[i] = T[i + 12];
    }
    return m;
}

inline M34 m_rigid_inverse(const M34& a) {  // [R t]^-1 = [R^T  -R^T t]
    M34 m{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.r[3 * i + j] = a.r[3 * j + i];
    for (int i = 0; i < 3; ++i) m.t[i] = -(m.r[3 * i] * a.t[0] + m.r[3 * i + 1] * a.t[1] + m.r[3 * i + 2] * a.t[2]);
    return m;
}

inline M34 m_rot_transpose(const M34& a) {  // inverse of a pure rotation
    M34 m{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.r[3 * i + j] = a.r[3 * j + i];
    return m;
}

// Rotations.jl UnitQuaternion(w, x, y, z) (normalising) -> RotMatrix
inline M34 m_quat(double w, double x, double y, double z) {
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n; x /= n; y /= n; z /= n;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, zw = w * z, xz = x * z, yw = y * w, yz = y * z, xw = w * x;
    M34 m{};
    m.r[0] = ww + xx - yy - zz; m.r[1] = 2 * (xy - zw);     m.r[2] = 2 * (xz + yw);
    m.r[3] = 2 * (xy + zw);     m.r[4] = ww - xx + yy - zz; m.r[5] = 2 * (yz - xw);
    m.r[6] = 2 * (xz - yw);     m.r[7] = 2 * (yz + xw);     m.r[8] = ww - xx - yy + zz;
    return m;
}

template <typename T>
void to_row12(const M34& m, T* out) {
    for (int i = 0; i < 3; ++i) {
        out[4 * i + 0] = (T)m.r[3 * i + 0];
        out[4 * i + 1] = (T)m.r[3 * i + 1];
        out[4 * i + 2] = (T)m.r[3 * i + 2];
        out[4 * i + 3] = (T)m.t[i];
    }
}

}  // namespace kinhip
