// mcbrat_camera_ctx.h -- what the backward camera (mcbrat_camera.hip, a translation unit of its own) is shown of a context.
// mcbrat_ctx is private to mcbrat_api.hip; the two functions below are defined there.  mcbrat_camera_context waits for whatever
// the context has in flight, brings the context's own lazy table upload up to date where asked, and fills a view: flags, the
// host copies the camera builds its own device buffers from, and the parameter block as fill_params writes it, with the DENSE
// optical grids (the camera never reads bricks).  It changes no setting, no moment and no tally of the context.
#pragma once
#include <vector>

#include "mcbrat_device.h"

namespace mcbrat {

struct CameraContext {
  int device = 0, numCUs = 0;
  size_t ldsPerCU = 0;
  hipStream_t stream = nullptr;  // the context's current lane, idle when the view is handed out
  bool haveGrid = false, haveOptics = false, haveSource = false;
  bool solarDirectional = false;  // the Directional solar source (mcbrat_set_source_solar)
  bool brdfSurface = false;       // a surface description of kind 1 to 3
  bool haveInverseTables = false; // every component has one, uploaded (asked for with needTables)
  int nc = 0;
  int gridInLds = -1;              // option "cameraGridInLds" (mcbrat_sun_transmittance)
  int pathBinsInLds = 1;           // option "cameraPathBinsInLds" (mcbrat_render_camera_pathlengths)
  const std::vector<double> *xe = nullptr, *ye = nullptr, *ze = nullptr;
  // forward tables per component as mcbrat_set_forward_table stored them ([nEntries][nAngles]; the original ones of a hybrid pair)
  const std::vector<std::vector<float>> *fwd = nullptr;
  const std::vector<int> *fwdNAngles = nullptr, *fwdNEntries = nullptr, *maxPfi = nullptr;
  DevParams p;  // valid where haveGrid && haveOptics
};

}  // namespace mcbrat

// 0, or 1 with the context's error text set (a failed synchronisation or table upload)
int mcbrat_camera_context(mcbrat_ctx *c, mcbrat::CameraContext *out, bool needTables);
// sets mcbrat_last_error and returns 1
int mcbrat_camera_fail(mcbrat_ctx *c, const char *msg);
