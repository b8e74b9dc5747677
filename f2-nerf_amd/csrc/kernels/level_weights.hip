// level_weights.hip -- the coarse-to-fine weights of the encoding's levels (f2n_level_weights).
// Host arithmetic only: nothing here touches the device.  The reference has no counterpart: its
// Hash3DAnchored::Query (src/hash_3d_anchored.cpp:79-87) feeds every level to the head at full weight.
#include "common.hiph"

#include <cmath>

extern "C" int f2n_level_weights(double alpha, int L, float * w_host, int * l_active)
{
  if (L < 1 || L > F2N_MAX_LEVELS || !w_host || !l_active) return F2N_E_INVALID_ARG;
  if (!std::isfinite(alpha) || alpha < 1.0) return F2N_E_INVALID_ARG;
  if (alpha > (double)L) alpha = (double)L;
  const double pi = 3.14159265358979323846;
  int last = 0;  // alpha >= 1: level 0 always speaks
  for (int l = 0; l < L; l++) {
    const double d = alpha - (double)l;
    double w;
    if (d <= 0.0)
      w = 0.0;
    else if (d < 1.0)
      w = (1.0 - std::cos(pi * d)) * 0.5;
    else
      w = 1.0;
    w_host[l] = (float)w;
    if (w_host[l] != 0.f) last = l;
  }
  *l_active = last + 1;
  return F2N_OK;
}
