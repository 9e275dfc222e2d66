"""kid_amd -- MI355X-native Thompson-09n column microphysics for the KiD driver.

One hot path of EnverRamirez/KiD (module_mp_thompson09n.f90 / mphys_thompson09n.f90)
as hand-written HIP kernels for gfx950 behind a C ABI (include/kidmp.h).
"""
from .thompson import (KidmpError, ThompsonMP, ThompsonMulti, mp_thompson, thompson_init, STATE_NAMES,  # noqa: F401
                       FORCING_NAMES, RATE_NAMES, KID_FIELDS, KID_WORK_NAMES, lib_path, load_library, cache_read_file, cache_write_file,
                       limbs_to_sums, shard_bounds)
from .stats import LevelStats, level_stats, stats_chunks, stats_workspace_bytes  # noqa: F401
from .summary import SUMMARY_INPUTS, SUMMARY_NAMES, column_summary, column_summary_host  # noqa: F401
from .doppler import DOPPLER_INPUTS, DOPPLER_NAMES, doppler_moments, doppler_moments_host  # noqa: F401
from .lidar import LIDAR_INPUTS, LIDAR_NAMES, LIDAR_SUMMARY_NAMES, LidarCfg, lidar_profiles, lidar_profiles_host  # noqa: F401
from .fall import FALL_INPUTS, FALL_NAMES, fall_speeds, fall_speeds_host  # noqa: F401
from .brightband import BRIGHTBAND_INPUTS, BRIGHTBAND_NAMES, BrightBandCfg, bright_band, bright_band_host  # noqa: F401
from .mie import MIE_INPUTS, MIE_NAMES, MIE_ROWS, MIE_SPECIES, MieCfg, MieTable, mie_bins, mie_radar, mie_radar_host, mie_sphere  # noqa: F401
# (the function radiometer.radiometer is not re-exported: the name is the submodule's; ThompsonMP.radiometer calls it)
from .radiometer import (RADIOMETER_INPUTS, RADIOMETER_NAMES, RADIOMETER_ROWS, RADIOMETER_SUMMARY_NAMES, RadiometerCfg, RadiometerTable,  # noqa: F401
                         radiometer_bins, radiometer_host, radiometer_sphere)
from .multichannel import MAX_CHANNELS, mie_radar_multi, mie_radar_multi_host, multichannel_tile, radiometer_multi, radiometer_multi_host  # noqa: F401
# (the function polarimetric.polarimetric is not re-exported either: ThompsonMP.polarimetric calls it)
from .polarimetric import POL_INPUTS, POL_NAMES, POL_ROWS, POL_SCALARS, PolCfg, PolTable, pol_bins, pol_spheroid, polarimetric_host  # noqa: F401
# (the function scan.scan IS re-exported, so the attribute kid_amd.scan is the function: reach the submodule with
# `from kid_amd.scan import ...` or importlib.import_module("kid_amd.scan"))
from .scan import SCAN_NAMES, ScanCfg, rhi_rays, scan  # noqa: F401
from .dspectrum import DSPECTRUM_INPUTS, DSPECTRUM_NAMES, doppler_spectrum, doppler_spectrum_host, velocity_grid  # noqa: F401
from .specproc import SPECPROC_NAMES, SpecCfg, spectrum_process  # noqa: F401
from .spectra import SPECTRA_INPUTS, SPECTRA_PARAMS, SPECTRA_SPECIES, default_grid, size_spectra, size_spectra_host  # noqa: F401
from .kinematic import ADVECT_OUTPUTS, advect, run, update  # noqa: F401
from .advection import SCHEMES as ADVECTION_SCHEMES  # noqa: F401
from .slab import advect_slab, run_slab, streamfunction_flow  # noqa: F401
from .aerosol import (AEROSOL_FIELDS, advect_aero, advect_slab_aero, kid_interface_aero, run_aero, run_slab_aero,  # noqa: F401
                      update_aero)
