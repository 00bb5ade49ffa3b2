// Host-side helpers of the kernel launchers: the set of supported hidden widths and the size of a persistent grid.
#pragma once
#include <type_traits>

#include "fenerf_internal.h"

namespace fenerf {

// The hidden widths the kernels are instantiated for.  Calls f(std::integral_constant<int, H>{}) for the model's (padded) width and
// returns its result; FENERF_E_UNSUPPORTED for any other width.
template <class F>
int dispatch_width(int H, F&& f) {
  switch (H) {
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 96: return f(std::integral_constant<int, 96>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 192: return f(std::integral_constant<int, 192>{});
    case 256: return f(std::integral_constant<int, 256>{});
  }
  return fail(FENERF_E_UNSUPPORTED, "unsupported hidden_dim");
}
// ... crossed with "the model has a feature grid": f(std::integral_constant<int, H>{}, std::bool_constant<GRID>{})
template <class F>
int dispatch_width(int H, bool grid, F&& f) {
  return dispatch_width(H, [&](auto h) { return grid ? f(h, std::true_type{}) : f(h, std::false_type{}); });
}

// Workgroups of a persistent kernel: one per `per_block` units of work, at most `cus` (one per compute unit), at least one.  `cus` is
// the caller's decision: the forward launchers pass the device's m->num_cus, the backward launchers launch_cus(m), which
// fenerf_set_cu_budget lowers (include/fenerf.h).
inline unsigned persistent_blocks(long long units, int per_block, long long cus) {
  long long blocks = (units + per_block - 1) / per_block;
  if (blocks > cus) blocks = cus;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

}  // namespace fenerf
