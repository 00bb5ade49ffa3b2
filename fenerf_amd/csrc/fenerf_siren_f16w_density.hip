// The plain-density instantiations of the forward kernel (fenerf_siren_f16w.hip, PASS = 3: labels and sigma without the colour branch,
// compact rows), as a translation unit of their own: the forward kernel's unit is the longest compile of the build as it
// is, and the two units compile side by side.  Defines fenerf::launch_siren16w_plain_density only.
#define FENERF_F16W_DENSITY_TU 1
#include "fenerf_siren_f16w.hip"
