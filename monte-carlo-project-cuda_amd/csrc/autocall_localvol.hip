// autocall_localvol.hip — worst-of autocallable notes under per-asset local-volatility surfaces for gfx950: the
// launcher's checks and the fp64 kernels (D = 1..8, two knock-in variants).  The fp32 kernels are compiled in
// autocall_localvol_f32.hip; the kernel itself is in autocall_localvol_impl.hpp.
#include "autocall_localvol_impl.hpp"

namespace mcamd {

hipError_t launch_autocall_localvol_f64(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                        const FinishSpec &finish, hipStream_t stream)
{
    return launch_autocall_localvol_t<double>(job, d_partials, grid, finish, stream);
}

hipError_t launch_autocall_localvol(const AutocallLocalVolJob &job, double *d_partials, uint32_t grid,
                                    const FinishSpec &finish, hipStream_t stream)
{
    if (!finish_ok(finish, grid)) return hipErrorInvalidValue;
    const uint32_t n_steps = job.paths.n_steps;
    if (!autocall_schedule_ok(job.schedule, n_steps)) return hipErrorInvalidValue;
    if (job.d < 1 || job.d > kBasketMaxAssets) return hipErrorInvalidValue;
    uint64_t nodes = 0;                // the D tables share one LDS allocation: no index may leave its own table
    for (int j = 0; j < job.d; ++j) {
        if (!lv_grid_ok(job.surface[j], n_steps)) return hipErrorInvalidValue;
        nodes += static_cast<uint64_t>(job.surface[j].n_t) * job.surface[j].n_x;
        if (nodes > kLocalVolMaxNodes) return hipErrorInvalidValue;
    }
    return job.paths.precision == 32 ? launch_autocall_localvol_f32(job, d_partials, grid, finish, stream)
                               : launch_autocall_localvol_f64(job, d_partials, grid, finish, stream);
}

}  // namespace mcamd
