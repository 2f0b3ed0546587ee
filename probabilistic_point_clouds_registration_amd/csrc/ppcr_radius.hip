// Translation unit of radius_moments_kernel (ppcr_radius.hip.h): its six instantiations and the one function that launches
// them.  Built without packed f32 arithmetic (build.py), unlike the rest of the library, whose objects stay as they were.
#include "ppcr_radius.hip.h"

namespace ppcr {
namespace dev {

void launch_radius_moments(const RadiusLaunch &a)
{
#define PPCR_RADIUS(TMc, ONEc)                                                                                                 \
    radius_moments_kernel<TMc, ONEc><<<a.blocks, kBlock, 0, a.stream>>>(a.src, a.ns, a.tgt, a.cell_start, a.g, a.r2, a.P, a.md, \
                                                                         a.partials, a.pair_counts)
    if (a.tm == 0) {
        if (a.onepass) PPCR_RADIUS(0, true);
        else PPCR_RADIUS(0, false);
    } else if (a.tm == 8) {
        if (a.onepass) PPCR_RADIUS(8, true);
        else PPCR_RADIUS(8, false);
    } else {
        if (a.onepass) PPCR_RADIUS(-1, true);
        else PPCR_RADIUS(-1, false);
    }
#undef PPCR_RADIUS
}

}  // namespace dev
}  // namespace ppcr
