// vw_launch.h -- shared by the launcher units vw_fwd.hip / vw_inv.hip / vw_lvl.hip, each compiled once
// per element type (the Makefile passes -DVW_T=double or -DVW_T=float).
#pragma once
#include "vw_device.h"

#ifndef VW_T
#error "compile with -DVW_T=double or -DVW_T=float"
#endif

namespace vw {

// VW_TAP_LIST, the unrolled tap counts: vw_taps.h (through vw_internal.h)

}  // namespace vw
