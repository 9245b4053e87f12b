// The bit-exact fit kernels of fit_kernels.hpp for fields of kind kFieldAnalytic: 32 fit_kernel, 4 fit_multi_kernel, 4 field_kernel.
// A unit per kind and nothing else in it, so that the three compile side by side.
#include "fit_kernels.hpp"

namespace hpsdf {

HPSDF_FIT_KIND_UNIT(, kFieldAnalytic)

}  // namespace hpsdf
