// Prints the backward camera's pixel mapping (mcbrat3d_amd/csrc/mcbrat_camera_ray.h) for the camera given on the command line:
//   camera_ray_dump kind npx npy mu phiDeg xLo xHi yLo yHi z  px py pz  lx ly lz  ux uy uz  fovXDeg
// "refused: <text>" for a camera the mapping refuses, else one line per pixel and per (u, v) in {0, 0.5, 1}^2:
//   i j u v  ox oy oz  dx dy dz
// A stand-alone host program (plain C++, no HIP): tests/test_camera_host.py builds it with the address and undefined-behaviour
// sanitizers and holds the lines to the closed forms written out in numpy.
#include <cstdio>
#include <cstdlib>

#include "../mcbrat3d_amd/csrc/mcbrat_camera_ray.h"

int main(int argc, char **argv) {
  if (argc != 21) {
    fprintf(stderr, "usage: camera_ray_dump kind npx npy mu phiDeg xLo xHi yLo yHi z px py pz lx ly lz ux uy uz fovXDeg\n");
    return 2;
  }
  mcbrat_camera cam = {};
  cam.kind = atoi(argv[1]); cam.npx = atoi(argv[2]); cam.npy = atoi(argv[3]);
  cam.jitter = 1; cam.gridInLds = -1;
  cam.mu = (float)atof(argv[4]); cam.phiDeg = (float)atof(argv[5]);
  cam.xLo = atof(argv[6]); cam.xHi = atof(argv[7]); cam.yLo = atof(argv[8]); cam.yHi = atof(argv[9]); cam.z = atof(argv[10]);
  for (int a = 0; a < 3; ++a) {
    cam.position[a] = atof(argv[11 + a]);
    cam.look[a] = atof(argv[14 + a]);
    cam.up[a] = atof(argv[17 + a]);
  }
  cam.fovXDeg = (float)atof(argv[20]);
  if (const char *msg = mcbrat::camera_refusal(cam)) {
    printf("refused: %s\n", msg);
    return 0;
  }
  mcbrat::CameraGeometry g;
  mcbrat::camera_geometry(cam, g);
  const double uv[3] = {0.0, 0.5, 1.0};
  for (int j = 0; j < cam.npy; ++j)
    for (int i = 0; i < cam.npx; ++i)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double o[3], d[3];
          mcbrat::camera_ray(g, i, j, uv[a], uv[b], o, d);
          printf("%d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", i, j, uv[a], uv[b], o[0], o[1], o[2], d[0], d[1], d[2]);
        }
  return 0;
}
