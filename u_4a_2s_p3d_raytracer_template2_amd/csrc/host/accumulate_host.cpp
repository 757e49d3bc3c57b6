// accumulate_host.cpp -- the reprojection of p3d_accumulate, of p3d_accumulate_moving and of p3d_accumulate_variance in plain
// loops on the host: DESIGN "Temporal accumulation", "Accumulation through moved primitives" and "Variance-guided denoising"
// read operation by operation, float arithmetic without contraction (HFLAGS: -ffp-contract=off).  What the device kernels
// (../accumulate.hip) are compared against, bit for bit; it shares no code with them.
#include "accumulate_host.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace p3d_host {

namespace {

inline bool valid_depth(float z) { return std::isfinite(z) && z > 0.0f; }

// what a frame looks back at: one frame of planes and the camera they were seen through
struct Previous {
    const float *color, *depth, *normal, *length;
    const int32_t* hit;
    const p3d_camera* cam;
};

// the geometry of p3d_accumulate_moving for one frame: the records it was rendered with and those of the frame it looks back at
struct Moved {
    uint32_t n_prims;
    const uint32_t* type;
    const float *cur, *prev;        // [n_prims][12]
};

// the moments of p3d_accumulate_variance for one frame: those of the frame looked back at ([res_y][res_x][2]; read with a
// previous frame only) and the frame's two outputs, each of which may be NULL
struct Variance {
    const float* prev_moments;
    float *out_moments, *out_variance;
};

inline float lum(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
inline float max0(float v) { return v > 0.0f ? v : 0.0f; }

inline float dot3(const float* p, const float* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
inline bool same_words(const float* a, const float* b, int n) { return std::memcmp(a, b, 4 * (size_t)n) == 0; }

// P_prev of p3d_accumulate_moving for the point P on primitive I: written to Q.  false: a changed plane, no history.
bool previous_point(const Moved& m, int32_t I, const float* P, float* Q) {
    for (int k = 0; k < 3; k++) Q[k] = P[k];
    if (I < 0 || (uint32_t)I >= m.n_prims) return true;
    const float *a = m.cur + 12 * (size_t)I, *b = m.prev + 12 * (size_t)I;
    switch (m.type[I]) {
    case P3D_SPHERE: {
        if (same_words(a, b, 4)) return true;
        const float s = b[3] / a[3];
        for (int k = 0; k < 3; k++) { const float t = (P[k] - a[k]) * s; Q[k] = b[k] + t; }
        return true;
    }
    case P3D_TRIANGLE: {
        if (same_words(a, b, 9)) return true;
        float e1[3], e2[3], w[3];
        for (int k = 0; k < 3; k++) { e1[k] = a[3 + k] - a[k]; e2[k] = a[6 + k] - a[k]; w[k] = P[k] - a[k]; }
        const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), w1 = dot3(w, e1), w2 = dot3(w, e2);
        const float m1 = d11 * d22, m2 = d12 * d12;
        const float den = m1 - m2;
        const float b1 = d22 * w1, b2 = d12 * w2, g1 = d11 * w2, g2 = d12 * w1;
        const float beta = (b1 - b2) / den, gamma = (g1 - g2) / den;
        for (int k = 0; k < 3; k++) {
            const float f1 = b[3 + k] - b[k], f2 = b[6 + k] - b[k];
            const float t1 = f1 * beta, t2 = f2 * gamma;
            const float u = b[k] + t1;
            Q[k] = u + t2;
        }
        return true;
    }
    case P3D_BOX: {
        if (same_words(a, b, 6)) return true;
        for (int k = 0; k < 3; k++) {
            const float e = a[3 + k] - a[k];
            const float t = e != 0.0f ? (P[k] - a[k]) / e : 0.0f;
            const float u = (b[3 + k] - b[k]) * t;
            Q[k] = b[k] + u;
        }
        return true;
    }
    default:
        return same_words(a, b, 4);
    }
}

// one frame: C, Z, N, I its planes; prev NULL for a frame with nothing to look back at.  out_c may be C.  moved: NULL for
// p3d_accumulate; else I is not NULL and out_xy (or NULL) receives p3d_accumulate_moving's prev_xy.  var: NULL, or the moments
// of p3d_accumulate_variance, gathered by the same taps; its variance is the temporal one (0 where Z is not valid).
void accumulate_frame(const p3d_accumulate_params& p, const p3d_camera& cam, const float* C, const float* Z, const float* N,
                      const int32_t* I, const Previous* prev, float* out_c, float* out_l, const Moved* moved = nullptr, float* out_xy = nullptr,
                      const Variance* var = nullptr) {
    const int W = p.res_x, H = p.res_y;
    const float rx = (float)W, ry = (float)H;
    float uw[3], vh[3], vz[3];
    for (int k = 0; k < 3; k++) { uw[k] = cam.u[k] * cam.w; vh[k] = cam.v[k] * cam.h; vz[k] = cam.n[k] * -cam.plane_dist; }
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            const float c0[3] = {C[3 * pi], C[3 * pi + 1], C[3 * pi + 2]};
            float o[3] = {c0[0], c0[1], c0[2]}, len = 1.0f;
            const float l0 = var ? lum(c0) : 0.0f;
            float om[2] = {l0, l0 * l0};
            float xy[2];
            const uint32_t quiet_nan[2] = {0x7FC00000u, 0x7FC00000u};
            std::memcpy(xy, quiet_nan, sizeof xy);
            [&] {
                if (!prev) return;
                const float z = Z[pi];
                if (!valid_depth(z)) return;
                const p3d_camera& pc = *prev->cam;
                // 1. Camera::PrimaryRay((x + 0.5, y + 0.5)), RT/camera.h:91-108
                const float fx = ((float)x + 0.5f) / rx - 0.5f, fy = ((float)y + 0.5f) / ry - 0.5f;
                float D[3], d[3], P[3], q[3];
                for (int k = 0; k < 3; k++) { const float vx = uw[k] * fx, vy = vh[k] * fy; const float t = vx + vy; D[k] = t + vz[k]; }
                const float s0 = D[0] * D[0], s1 = D[1] * D[1], s2 = D[2] * D[2];
                const float l = 1.0f / std::sqrt((s0 + s1) + s2);
                for (int k = 0; k < 3; k++) { d[k] = D[k] * l; const float t = d[k] * z; P[k] = cam.eye[k] + t; }
                float Q[3] = {P[0], P[1], P[2]};
                if (moved && !previous_point(*moved, I[pi], P, Q)) return;
                for (int k = 0; k < 3; k++) q[k] = Q[k] - pc.eye[k];
                // 2. the projection into the previous camera
                const float a = (q[0] * pc.u[0] + q[1] * pc.u[1]) + q[2] * pc.u[2];
                const float b = (q[0] * pc.v[0] + q[1] * pc.v[1]) + q[2] * pc.v[2];
                const float c = -((q[0] * pc.n[0] + q[1] * pc.n[1]) + q[2] * pc.n[2]);
                if (!(c > 0.0f)) return;
                const float s = c / pc.plane_dist;
                const float gx = a / (pc.w * s), gy = b / (pc.h * s);
                const float px = (gx + 0.5f) * rx - 0.5f, py = (gy + 0.5f) * ry - 0.5f;
                if (!(px > -1.0f && px < rx && py > -1.0f && py < ry)) return;
                xy[0] = px; xy[1] = py;
                const float x0f = std::floor(px), y0f = std::floor(py);
                const float tx = px - x0f, ty = py - y0f;
                const long x0 = (long)x0f, y0 = (long)y0f;
                const float dist = std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
                const float lim = p.depth_tolerance * dist;
                // 3. the taps
                const float ux = 1.0f - tx, uy = 1.0f - ty;
                const float wgt[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
                const float* n = N + 3 * pi;
                const bool ids = I && prev->hit;
                float sum[3] = {0.0f, 0.0f, 0.0f}, sl = 0.0f, sw = 0.0f, sm[2] = {0.0f, 0.0f};
                for (int t = 0; t < 4; t++) {
                    const long qx = x0 + (t & 1), qy = y0 + (t >> 1);
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t qi = (size_t)qy * W + (size_t)qx;
                    const float zq = prev->depth[qi];
                    if (!valid_depth(zq)) continue;
                    if (!(std::fabs(zq - dist) <= lim)) continue;
                    const float* nq = prev->normal + 3 * qi;
                    const float dn = (n[0] * nq[0] + n[1] * nq[1]) + n[2] * nq[2];
                    if (!(dn >= p.normal_min)) continue;
                    if (ids && prev->hit[qi] != I[pi]) continue;
                    for (int k = 0; k < 3; k++) { const float m = wgt[t] * prev->color[3 * qi + k]; sum[k] = sum[k] + m; }
                    const float ml = wgt[t] * prev->length[qi];
                    sl = sl + ml;
                    if (var)
                        for (int k = 0; k < 2; k++) { const float mm = wgt[t] * var->prev_moments[2 * qi + k]; sm[k] = sm[k] + mm; }
                    sw = sw + wgt[t];
                }
                // 4. the blend
                if (!(sw > 0.0f)) return;
                float ln = sl / sw + 1.0f;
                if (ln > p.max_history) ln = p.max_history;
                const float alpha = 1.0f / ln;
                for (int k = 0; k < 3; k++) { const float h = sum[k] / sw; const float m = (c0[k] - h) * alpha; o[k] = h + m; }
                if (var)
                    for (int k = 0; k < 2; k++) { const float h = sm[k] / sw; const float m = (om[k] - h) * alpha; om[k] = h + m; }
                len = ln;
            }();
            if (out_c) { out_c[3 * pi] = o[0]; out_c[3 * pi + 1] = o[1]; out_c[3 * pi + 2] = o[2]; }
            if (out_l) out_l[pi] = len;
            if (out_xy) { out_xy[2 * pi] = xy[0]; out_xy[2 * pi + 1] = xy[1]; }
            if (var && var->out_moments) { var->out_moments[2 * pi] = om[0]; var->out_moments[2 * pi + 1] = om[1]; }
            if (var && var->out_variance) {
                const float sq = om[0] * om[0];
                var->out_variance[pi] = valid_depth(Z[pi]) ? max0(om[1] - sq) : 0.0f;
            }
        }
    }
}

// the spatial estimate of p3d_accumulate_variance for one frame: C, Z, N its INPUT planes, L its OUTPUT length; pixels with
// a valid Z and L < min_temporal whose taps carry weight get their variance replaced
void spatial_variance_frame(const p3d_accumulate_params& p, const p3d_accumulate_variance_params& vp, const float* C, const float* Z,
                            const float* N, const float* L, float* variance) {
    const int W = p.res_x, H = p.res_y, R = vp.radius;
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            const float zp = Z[pi];
            if (!valid_depth(zp) || !(L[pi] < vp.min_temporal)) continue;
            const float inv_z = 1.0f / (vp.sigma_depth * zp);
            const float* np = N + 3 * pi;
            float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
            for (int dy = -R; dy <= R; dy++) {
                for (int dx = -R; dx <= R; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t qi = (size_t)qy * W + (size_t)qx;
                    const float zq = Z[qi];
                    if (!valid_depth(zq)) continue;
                    const float tz = max0(1.0f - std::fabs(zq - zp) * inv_z);
                    const float wz = tz * tz;
                    float wn = max0(dot3(np, N + 3 * qi));
                    for (int j = 0; j < vp.normal_power_log2; j++) wn = wn * wn;
                    const float w = wz * wn;
                    const float lq = lum(C + 3 * qi);
                    const float t1 = w * lq;
                    s1 = s1 + t1;
                    const float l2 = lq * lq;
                    const float t2 = w * l2;
                    s2 = s2 + t2;
                    sw = sw + w;
                }
            }
            if (!(sw > 0.0f)) continue;
            const float a = s1 / sw, b = s2 / sw;
            const float sq = a * a;
            variance[pi] = max0(b - sq);
        }
    }
}

}  // namespace

namespace {

// what p3d_accumulate_variance adds to a sequence
struct VarianceSequence {
    const p3d_accumulate_variance_params* params;
    const float* history_moments;
    float *out_moments, *out_variance;
};

// the entries: motion NULL for accumulate(), var NULL for all but accumulate_variance()
void accumulate_sequence(const p3d_accumulate_params& p, const p3d_accumulate_frames& fr, const p3d_accumulate_history* history,
                         const p3d_accumulate_motion* motion, float* out_rgb32f, float* out_length, float* out_prev_xy,
                         const VarianceSequence* var = nullptr) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y;
    // an output the caller does not want is still what the next frame looks back at
    std::vector<float> own_c(out_rgb32f ? 0 : 3 * frame * p.n_frames), own_l(out_length ? 0 : frame * p.n_frames);
    float* oc = out_rgb32f ? out_rgb32f : own_c.data();
    float* ol = out_length ? out_length : own_l.data();
    std::vector<float> own_m(var && !var->out_moments ? 2 * frame * p.n_frames : 0);
    float* om = !var ? nullptr : var->out_moments ? var->out_moments : own_m.data();
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
        Previous prev, *pp = nullptr;
        if (f > 0) {
            prev = {oc + 3 * (f - 1) * frame, fr.depth + (f - 1) * frame, fr.normal + 3 * (f - 1) * frame, ol + (f - 1) * frame,
                    fr.hit_id ? fr.hit_id + (f - 1) * frame : nullptr, &fr.cams[f - 1]};
            pp = &prev;
        } else if (history) {
            prev = {history->rgb32f, history->depth, history->normal, history->length, history->hit_id, history->cam};
            pp = &prev;
        }
        Moved moved, *mp = nullptr;
        if (motion) {
            const size_t records = 12 * (size_t)motion->n_prims;
            moved = {motion->n_prims, motion->prim_type, motion->prim_data + f * records,
                     f > 0 ? motion->prim_data + (f - 1) * records : motion->history_prim_data};
            mp = &moved;
        }
        Variance v, *vp = nullptr;
        if (var) {
            v = {f > 0 ? om + 2 * (f - 1) * frame : var->history_moments, om + 2 * f * frame,
                 var->out_variance ? var->out_variance + f * frame : nullptr};
            vp = &v;
        }
        accumulate_frame(p, fr.cams[f], fr.rgb32f + 3 * f * frame, fr.depth + f * frame, fr.normal + 3 * f * frame,
                         fr.hit_id ? fr.hit_id + f * frame : nullptr, pp, oc + 3 * f * frame, ol + f * frame, mp,
                         out_prev_xy ? out_prev_xy + 2 * f * frame : nullptr, vp);
        if (var && var->out_variance)
            spatial_variance_frame(p, *var->params, fr.rgb32f + 3 * f * frame, fr.depth + f * frame, fr.normal + 3 * f * frame,
                                   ol + f * frame, var->out_variance + f * frame);
    }
}

}  // namespace

void accumulate(const p3d_accumulate_params& p, const p3d_accumulate_frames& fr, const p3d_accumulate_history* history,
                float* out_rgb32f, float* out_length) {
    accumulate_sequence(p, fr, history, nullptr, out_rgb32f, out_length, nullptr);
}

void accumulate_moving(const p3d_accumulate_params& p, const p3d_accumulate_frames& fr, const p3d_accumulate_history* history,
                       const p3d_accumulate_motion& motion, float* out_rgb32f, float* out_length, float* out_prev_xy) {
    accumulate_sequence(p, fr, history, &motion, out_rgb32f, out_length, out_prev_xy);
}

void accumulate_variance(const p3d_accumulate_params& p, const p3d_accumulate_variance_params& vp, const p3d_accumulate_frames& fr,
                         const p3d_accumulate_history* history, const float* history_moments, const p3d_accumulate_motion* motion,
                         float* out_rgb32f, float* out_length, float* out_moments, float* out_variance, float* out_prev_xy) {
    const VarianceSequence var = {&vp, history_moments, out_moments, out_variance};
    accumulate_sequence(p, fr, history, motion, out_rgb32f, out_length, motion ? out_prev_xy : nullptr, &var);
}

}  // namespace p3d_host
