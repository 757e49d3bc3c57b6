// accumulate_host.cpp -- the reprojection of p3d_accumulate in plain loops on the host: DESIGN "Temporal accumulation" read
// operation by operation, float arithmetic without contraction (HFLAGS: -ffp-contract=off).  What the device kernel
// (../accumulate.hip) is compared against, bit for bit; it shares no code with it.
#include "accumulate_host.h"

#include <cmath>
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

// one frame: C, Z, N, I its planes; prev NULL for a frame with nothing to look back at.  out_c may be C.
void accumulate_frame(const p3d_accumulate_params& p, const p3d_camera& cam, const float* C, const float* Z, const float* N,
                      const int32_t* I, const Previous* prev, float* out_c, float* out_l) {
    const int W = p.res_x, H = p.res_y;
    const float rx = (float)W, ry = (float)H;
    float uw[3], vh[3], vz[3];
    for (int k = 0; k < 3; k++) { uw[k] = cam.u[k] * cam.w; vh[k] = cam.v[k] * cam.h; vz[k] = cam.n[k] * -cam.plane_dist; }
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            const float c0[3] = {C[3 * pi], C[3 * pi + 1], C[3 * pi + 2]};
            float o[3] = {c0[0], c0[1], c0[2]}, len = 1.0f;
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
                for (int k = 0; k < 3; k++) { d[k] = D[k] * l; const float t = d[k] * z; P[k] = cam.eye[k] + t; q[k] = P[k] - pc.eye[k]; }
                // 2. the projection into the previous camera
                const float a = (q[0] * pc.u[0] + q[1] * pc.u[1]) + q[2] * pc.u[2];
                const float b = (q[0] * pc.v[0] + q[1] * pc.v[1]) + q[2] * pc.v[2];
                const float c = -((q[0] * pc.n[0] + q[1] * pc.n[1]) + q[2] * pc.n[2]);
                if (!(c > 0.0f)) return;
                const float s = c / pc.plane_dist;
                const float gx = a / (pc.w * s), gy = b / (pc.h * s);
                const float px = (gx + 0.5f) * rx - 0.5f, py = (gy + 0.5f) * ry - 0.5f;
                if (!(px > -1.0f && px < rx && py > -1.0f && py < ry)) return;
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
                float sum[3] = {0.0f, 0.0f, 0.0f}, sl = 0.0f, sw = 0.0f;
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
                    sw = sw + wgt[t];
                }
                // 4. the blend
                if (!(sw > 0.0f)) return;
                float ln = sl / sw + 1.0f;
                if (ln > p.max_history) ln = p.max_history;
                const float alpha = 1.0f / ln;
                for (int k = 0; k < 3; k++) { const float h = sum[k] / sw; const float m = (c0[k] - h) * alpha; o[k] = h + m; }
                len = ln;
            }();
            if (out_c) { out_c[3 * pi] = o[0]; out_c[3 * pi + 1] = o[1]; out_c[3 * pi + 2] = o[2]; }
            if (out_l) out_l[pi] = len;
        }
    }
}

}  // namespace

void accumulate(const p3d_accumulate_params& p, const p3d_accumulate_frames& fr, const p3d_accumulate_history* history,
                float* out_rgb32f, float* out_length) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y;
    // an output the caller does not want is still what the next frame looks back at
    std::vector<float> own_c(out_rgb32f ? 0 : 3 * frame * p.n_frames), own_l(out_length ? 0 : frame * p.n_frames);
    float* oc = out_rgb32f ? out_rgb32f : own_c.data();
    float* ol = out_length ? out_length : own_l.data();
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
        accumulate_frame(p, fr.cams[f], fr.rgb32f + 3 * f * frame, fr.depth + f * frame, fr.normal + 3 * f * frame,
                         fr.hit_id ? fr.hit_id + f * frame : nullptr, pp, oc + 3 * f * frame, ol + f * frame);
    }
}

}  // namespace p3d_host
