// mcbrat_camera_ray.h -- the one statement of the backward camera's pixel mapping: which point and which
// backward direction belong to the position (i + u, j + v) of an image.  camera_kernel (mcbrat_camera.hip) and the host function
// mcbrat_camera_ray call the same camera_ray() over the same CameraGeometry, which camera_geometry() derives from a
// mcbrat_camera on the host.  Plain C++ in double: no HIP header is needed to read it (tests/camera_ray_dump.cpp includes
// nothing else); under hipcc the two functions the kernel calls are __host__ __device__.
//
//   orthographic  the light arriving travels along t = (sin(theta) cos(phi), sin(theta) sin(phi), mu), mu = cos(theta) -- the
//                 convention of intensityMus / intensityPhis.  Pixel (i, j) starts at
//                 (xLo + (i + u)(xHi - xLo) / npx, yLo + (j + v)(yHi - yLo) / npy, z) and walks backward along -t.
//   pinhole       right = normalize(look x up), trueUp = right x lookHat,
//                 s = (2 (i + u) / npx - 1) tan(fov / 2), t = (2 (j + v) / npy - 1) tan(fov / 2) npy / npx,
//                 line of sight = normalize(lookHat + s right + t trueUp): j grows upward.  Every pixel starts at `position`.
#pragma once
#include <math.h>

#include "../../include/mcbrat.h"

#if defined(__HIPCC__)
#define MCBRAT_CAMERA_HD __host__ __device__
#else
#define MCBRAT_CAMERA_HD
#endif

namespace mcbrat {

struct CameraGeometry {
  int kind, npx, npy;
  double origin[3];   // pinhole: the position; orthographic: (xLo, yLo, z)
  double stepX, stepY; // orthographic: pixel size; pinhole: 2 tan(fov / 2) / npx (both axes: square pixels)
  double axis[3];     // orthographic: -t, the backward direction of every pixel; pinhole: lookHat
  double right[3], trueUp[3];  // pinhole
  double tanHalf, tanHalfY;    // pinhole: tan(fov / 2) and tan(fov / 2) npy / npx
};

// What is wrong with a camera that no context is needed to see, or NULL.  (Heights against the domain, and the tally budget,
// are mcbrat_render_camera's.)
inline const char *camera_refusal(const mcbrat_camera &cam) {
  if (cam.kind != 0 && cam.kind != 1) return "renderCamera: camera kind must be 0 (orthographic) or 1 (pinhole).";
  if (cam.npx < 1 || cam.npy < 1) return "renderCamera: the image needs at least one pixel in x and in y.";
  if (cam.gridInLds < -1 || cam.gridInLds > 1) return "renderCamera: gridInLds must be -1, 0 or 1.";
  if (cam.kind == 0) {
    if (!(fabs((double)cam.mu) <= 1.0) || cam.mu == 0.0f) return "renderCamera: the camera's mu must be in [-1, 1] and can't be 0 (directly sideways).";
    if (!(cam.phiDeg >= 0.0f && cam.phiDeg <= 360.0f)) return "renderCamera: the camera's phi must be between 0 and 360.";
    if (!(cam.xHi > cam.xLo) || !(cam.yHi > cam.yLo) || !isfinite(cam.xHi - cam.xLo) || !isfinite(cam.yHi - cam.yLo))
      return "renderCamera: degenerate footprint (xHi > xLo and yHi > yLo are needed).";
    if (!isfinite(cam.z)) return "renderCamera: the camera's height is not finite.";
  } else {
    if (!(cam.fovXDeg > 0.0f && cam.fovXDeg < 180.0f)) return "renderCamera: the field of view must be in (0, 180) degrees.";
    double l2 = 0.0, u2 = 0.0, c2 = 0.0;
    const double cx[3] = {cam.look[1] * cam.up[2] - cam.look[2] * cam.up[1], cam.look[2] * cam.up[0] - cam.look[0] * cam.up[2],
                          cam.look[0] * cam.up[1] - cam.look[1] * cam.up[0]};
    for (int a = 0; a < 3; ++a) { l2 += cam.look[a] * cam.look[a]; u2 += cam.up[a] * cam.up[a]; c2 += cx[a] * cx[a]; }
    if (!isfinite(l2) || !isfinite(u2) || !(l2 > 0.0) || !(u2 > 0.0)) return "renderCamera: look and up must be finite, non-zero vectors.";
    if (!(c2 > 1e-24 * l2 * u2)) return "renderCamera: look and up are parallel.";
    if (!isfinite(cam.position[0]) || !isfinite(cam.position[1]) || !isfinite(cam.position[2])) return "renderCamera: the camera's position is not finite.";
  }
  return 0;
}

// The geometry of a camera that camera_refusal() passes
inline void camera_geometry(const mcbrat_camera &cam, CameraGeometry &g) {
  const double kPi = 3.14159265358979323846;
  g = CameraGeometry();
  g.kind = cam.kind; g.npx = cam.npx; g.npy = cam.npy;
  if (cam.kind == 0) {
    const double mu = (double)cam.mu, phi = (double)cam.phiDeg * kPi / 180.0;
    const double sinTheta = sqrt(1.0 - mu * mu);
    g.axis[0] = -(sinTheta * cos(phi)); g.axis[1] = -(sinTheta * sin(phi)); g.axis[2] = -mu;
    g.origin[0] = cam.xLo; g.origin[1] = cam.yLo; g.origin[2] = cam.z;
    g.stepX = (cam.xHi - cam.xLo) / (double)cam.npx;
    g.stepY = (cam.yHi - cam.yLo) / (double)cam.npy;
    return;
  }
  const double ln = sqrt(cam.look[0] * cam.look[0] + cam.look[1] * cam.look[1] + cam.look[2] * cam.look[2]);
  for (int a = 0; a < 3; ++a) { g.axis[a] = cam.look[a] / ln; g.origin[a] = cam.position[a]; }
  double r[3] = {cam.look[1] * cam.up[2] - cam.look[2] * cam.up[1], cam.look[2] * cam.up[0] - cam.look[0] * cam.up[2],
                 cam.look[0] * cam.up[1] - cam.look[1] * cam.up[0]};
  const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int a = 0; a < 3; ++a) g.right[a] = r[a] / rn;
  g.trueUp[0] = g.right[1] * g.axis[2] - g.right[2] * g.axis[1];
  g.trueUp[1] = g.right[2] * g.axis[0] - g.right[0] * g.axis[2];
  g.trueUp[2] = g.right[0] * g.axis[1] - g.right[1] * g.axis[0];
  g.tanHalf = tan(0.5 * (double)cam.fovXDeg * kPi / 180.0);
  g.tanHalfY = g.tanHalf * (double)cam.npy / (double)cam.npx;
  g.stepX = g.stepY = 2.0 * g.tanHalf / (double)cam.npx;
}

// Origin and backward direction (unit) of the position (i + u, j + v) of the image
MCBRAT_CAMERA_HD inline void camera_ray(const CameraGeometry &g, int i, int j, double u, double v, double origin[3], double direction[3]) {
  if (g.kind == 0) {
    origin[0] = g.origin[0] + ((double)i + u) * g.stepX;
    origin[1] = g.origin[1] + ((double)j + v) * g.stepY;
    origin[2] = g.origin[2];
    direction[0] = g.axis[0]; direction[1] = g.axis[1]; direction[2] = g.axis[2];
    return;
  }
  const double s = (2.0 * ((double)i + u) / (double)g.npx - 1.0) * g.tanHalf;
  const double t = (2.0 * ((double)j + v) / (double)g.npy - 1.0) * g.tanHalfY;
  double d[3], n2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    d[a] = g.axis[a] + s * g.right[a] + t * g.trueUp[a];
    n2 += d[a] * d[a];
    origin[a] = g.origin[a];
  }
  const double inv = 1.0 / sqrt(n2);
  for (int a = 0; a < 3; ++a) direction[a] = d[a] * inv;
}

}  // namespace mcbrat
