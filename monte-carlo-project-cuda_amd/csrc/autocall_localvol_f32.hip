// autocall_localvol_f32.hip — the fp32 kernels of autocall_localvol_impl.hpp (D = 1..8, two knock-in variants), in a
// translation unit of their own so that the two precisions compile side by side.
#include "autocall_localvol_impl.hpp"

namespace mcamd {

hipError_t launch_autocall_localvol_f32(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                        const FinishSpec &finish, hipStream_t stream)
{
    return launch_autocall_localvol_t<float>(job, d_partials, grid, finish, stream);
}

}  // namespace mcamd
