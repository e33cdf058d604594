// dtof_world_to_pixel.h -- S, the 3 x 4 matrix that takes a world-space point to FILM pixel coordinates (dtof_scene_world_to_pixel, include/dtof.h): rows x, y, w of
// camera_to_sample o to_world^-1 (perspective_projection / orthographic_projection, include/mitsuba/render/sensor.h:226-299), the x and y rows scaled by the film
// size.  The crop factors are left out -- they only move the origin to the crop window -- so pix(P) is in the coordinates of a lane's sample_pos.  The depth row is
// absent, so near and far clip do not enter.  Plain C++ in double from the loader's float32 sensor; no HIP, no device.
#pragma once
#include <cmath>
#include <stdexcept>
#include "dtof_scene.h"

namespace dtof {

inline void world_to_pixel(const HostSensor &s, double out[12]) {
    const float *m = s.to_world;      // rows of 4: camera -> world, affine (an orthographic sensor's carries its scale)
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = a * c00 + b * c01 + c * c02;
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) throw std::runtime_error("the sensor's to_world is singular");
    // V = to_world^-1: the adjugate over the determinant, and -V3 t
    double V[3][4] = { { c00 / det, (c * h - b * i) / det, (b * f - c * e) / det, 0 },
                       { c01 / det, (a * i - c * g) / det, (c * d - a * f) / det, 0 },
                       { c02 / det, (b * g - a * h) / det, (a * e - b * d) / det, 0 } };
    const double t[3] = { m[3], m[7], m[11] };
    for (int r = 0; r < 3; ++r) V[r][3] = -(V[r][0] * t[0] + V[r][1] * t[1] + V[r][2] * t[2]);
    const double fw = s.film_w, fh = s.film_h, aspect = fw / fh;
    // behind the projection: X = cot x, Y = cot y, W = z (perspective; thinlens: its pinhole, the lens centre), X = x, Y = y, W = 1 (orthographic);
    // then translate(-1, -1 / aspect), scale(-1/2, -aspect / 2) and the film size
    const double cot = s.orthographic ? 1.0 : 1.0 / std::tan((double) (s.x_fov * .5f) * (M_PI / 180.0));
    double w[4] = { V[2][0], V[2][1], V[2][2], V[2][3] };
    if (s.orthographic) { w[0] = w[1] = w[2] = 0; w[3] = 1; }
    for (int k = 0; k < 4; ++k) {
        out[k] = (-0.5 * fw) * (cot * V[0][k] - w[k]);
        out[4 + k] = (-0.5 * aspect * fh) * (cot * V[1][k] - w[k] / aspect);
        out[8 + k] = w[k];
    }
}

}  // namespace dtof
