// The one pass loop of the plain-kernel stage's three families: unscaled and scaled (cmx_variants.hip) and the wide mapping
// (cmx_map_wide.hip).  Host code only.
#pragma once
#include "cmx_device.h"

namespace cmx {

// It carves D, M, U, Up from `scratch` (plain_node_doubles) and, if `exps` is not null, eD and eU from it
// (plain_exponent_ints), then walks a.chunk sites per pass.  Per pass: inside(pass); scalars(pass) if a site scalar is asked
// for (a family that does not serve them launches nothing; its error ends the loop at once); and -- only if `outside` --
// rest(pass): the family's outside part and what the caller launches on the finished vectors.
struct PlainPass {
  PlainArgs a;        // site0, nsites and the four vectors set
  int32_t *eD, *eU;   // null: unscaled
  unsigned gx;        // workgroups of 256 sites
};
template <class Inside, class Scalars, class Rest>
hipError_t plain_passes(const PlainArgs& a, size_t nsites_total, double* scratch, int32_t* exps, bool outside, Inside inside,
                        Scalars scalars, Rest rest) {
  const size_t per = plain_node_doubles(a.S, a.C, a.nn, a.chunk) / 4;
  PlainPass p{a, exps, exps ? exps + plain_exponent_ints(a.C, a.nn, a.chunk) / 2 : nullptr, 0};
  p.a.D = scratch; p.a.M = scratch + per; p.a.U = scratch + 2 * per; p.a.Up = scratch + 3 * per;
  for (p.a.site0 = 0; p.a.site0 < nsites_total; p.a.site0 += p.a.chunk) {
    p.a.nsites = p.a.chunk < nsites_total - p.a.site0 ? p.a.chunk : nsites_total - p.a.site0;
    p.gx = (unsigned)((p.a.nsites + 255) / 256);
    inside(p);
    if (p.a.logL || p.a.post_rate || p.a.rate_class)
      if (hipError_t e = scalars(p); e != hipSuccess) return e;
    if (outside) rest(p);
  }
  return hipSuccess;
}

}  // namespace cmx
