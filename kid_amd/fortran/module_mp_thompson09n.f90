!
! module_mp_thompson09n -- drop-in replacement for the reference module of the
! same name (/root/reference/module_mp_thompson09n.f90, "M:").  It keeps the two
! procedures the KiD adapter calls, with the reference's dummy lists:
!
!     thompson_init()                                   M:374
!     mp_thompson(qv1d, ..., kts, kte, dt, ii, jj)      M:1156-1177
!
! and adds the batched form of the adapter's `do i=1,nx` loop (W:54-246):
!
!     mp_thompson_batch(ncol, nz, dt, qv, ..., ppt)
!
! and the two diagnostics of the reference module a host model calls beside the step, with its dummy lists:
!
!     calc_refl10cm(qv1d, ..., dBZ, kts, kte, ii, jj)   M:4946-4952
!     calc_effectRad(t1d, ..., re_qs1d, kts, kte)       M:4834-4843
!
! Bodies are ISO_C_BINDING calls into libkidmp.so (include/kidmp.h), where the
! column physics runs as hand-written HIP kernels on an MI355X.  Arithmetic (kidmp_arith):
!   'p64'   (default) state arrays are copied to REAL(c_double) temporaries and the step runs in binary64 -- the
!           parity build; works whether KiD is compiled with 4-byte or 8-byte default REAL;
!   'p32n'  KiD's default 4-byte REAL only: the REAL arrays go to the GPU as they are and the kernel keeps the
!           reference's own split -- what it declares REAL in binary32, its DOUBLE PRECISION rates in binary64
!           (the reference as shipped);
!   'f32'   likewise, everything binary32.
!
! Like the reference it takes its switches from KiD's own modules:
! iiwarm, set_Nc (namelists, M:22), l_sediment and l_reuse_thompson_lookup (switches, M:20) and nx (parameters, M:23).
! l_reuse_thompson_lookup keeps the reference's meaning (M:3717-3729, M:3864-3895): a run_data/racg_thompson09.data /
! run_data/racs_thompson09.data that exists is READ when the switch is set; otherwise the tables are built (on the GPU)
! and WRITTEN there, in the reference's list-directed format (without a run_data directory nothing is written; the
! reference aborts in that case, M:3718).
!
! More than one GPU: kidmp_ndevices > 1 with kidmp_devices(1:kidmp_ndevices) (or the environment variable
! KIDMP_DEVICES = "0,1,2,..."): thompson_init builds the tables on every device and mp_thompson_batch spreads the
! columns over them in contiguous ranges (kidmp_batch_step_host_multi: one pipeline per device, the domain sums of the
! surface precipitation reduced with RCCL and left in kidmp_precip_sums).  'p64' arithmetic only.
!
! Side effects kept: the 36 process-rate diagnostics the reference emits from inside mp_thompson
! (M:2962-3124) are replayed after the batched call through KiD's own save_dg, same names, same
! order (per column, per level: 30 mixed-phase rates unless iiwarm, then 6 warm ones), same
! nx == 1 / nx > 1 call forms, and none for a column that took the no_micro early return
! (M:1540).  l_rate_diagnostics = .false. switches them off (big batches: the rate buffer is
! 36 profiles per column).  kidmp_device (or the environment variable KIDMP_DEVICE) selects the GPU.
!
module module_mp_thompson09n

  use iso_c_binding
  use switches, only: l_sediment, l_reuse_thompson_lookup
  use namelists, only: iiwarm, set_Nc
  use parameters, only: nx
  use diagnostics, only: save_dg, i_dgtime

  implicit none
  private

  public :: thompson_init, mp_thompson, mp_thompson_batch, mp_thompson_staging, thompson_finalize
  public :: kidmp_precip_sums_valid
  public :: calc_refl10cm, calc_refl10cm_batch
  public :: calc_effectRad, calc_effectRad_batch
  public :: mp_thompson_set_column_nc
  public :: column_summary_batch
  public :: fall_speeds_batch
  public :: doppler_moments_batch
  public :: size_spectra_batch
  public :: doppler_spectrum_batch
  public :: bright_band_batch
  public :: mie_radar_batch
  public :: polarimetric_batch
  public :: radiometer_batch
  public :: radiometer_multi_batch, mie_radar_multi_batch
  public :: lidar_profiles_batch
  public :: mp_thompson_kid_interface, mp_thompson_kid_staging
  logical, public :: is_aerosol_aware = .false.          ! M:28 (read at thompson_init)
  logical, public :: l_rate_diagnostics = .true.         ! replay the save_dg calls of M:2962-3124
  integer, public :: kidmp_device = 0                    ! HIP device ordinal of this process (one GPU)
  integer, public :: kidmp_ndevices = 1                  ! > 1: the columns are spread over kidmp_devices(1:kidmp_ndevices)
  integer, public :: kidmp_devices(8) = (/ 0, 1, 2, 3, 4, 5, 6, 7 /)
  ! domain sums (rain, snow, graupel, ice) of ppt after the last mp_thompson_batch call on several devices: the
  ! numerators of the nx-means of W:248-303, reduced over the devices with RCCL inside the library
  real(c_double), public :: kidmp_precip_sums(4) = 0.0_c_double
  character(64), public :: kidmp_cache_dir = 'run_data'  ! where the reference keeps its table cache (M:3710, M:3857)
  character(4), public :: kidmp_arith = 'p64 '           ! 'p64', or with 4-byte default REAL 'p32n' / 'f32'

  ! the diagnosed rates in the reference's emission order (M:2967-3119): 30 mixed-phase, then 6 warm
  integer, parameter :: NRATES = 36, NRATES_MIXED = 30
  character(7), parameter :: rate_names(NRATES) = (/ &
       'pri_inu', 'pri_ide', 'prs_ide', 'prs_sde', 'prg_gde', 'pri_wfz', 'prs_scw', 'prg_scw', 'prg_gcw', 'pri_ihm', &
       'pri_rfz', 'prs_iau', 'prs_sci', 'pri_rci', 'pni_inu', 'pni_ihm', 'pni_wfz', 'pni_rfz', 'pni_ide', 'pni_iau', &
       'pni_sci', 'pni_rci', 'prr_sml', 'prr_gml', 'pnr_rcs', 'pnr_rcg', 'pnr_rci', 'pnr_sml', 'pnr_gml', 'pnr_rfz', &
       'prr_wau', 'prr_rcw', 'prv_rev', 'pnr_wau', 'pnr_rev', 'pnr_rcr' /)

  type, bind(C) :: kidmp_cfg
     integer(c_int32_t) :: iiwarm
     integer(c_int32_t) :: l_sediment
     real(c_double)     :: set_Nc
     integer(c_int32_t) :: device
     integer(c_int32_t) :: is_aerosol_aware
  end type kidmp_cfg

  type, bind(C) :: kidmp_outputs                         ! kidmp_outputs / kidmp32_outputs: NULL = not wanted
     type(c_ptr) :: dbz, re_qc, re_qi, re_qs
  end type kidmp_outputs

  type, bind(C) :: kidmp_fall_out                        ! kidmp_fall_out / kidmp32_fall_out: [ncol][nz] each, NULL = not wanted
     type(c_ptr) :: vt_r, vt_nr, vt_i, vt_ni, vt_s, vt_g, flux_r, flux_i, flux_s, flux_g, flux_total
  end type kidmp_fall_out
  type, bind(C) :: kidmp_doppler_out                     ! kidmp_doppler_out / kidmp32_doppler_out: [ncol][nz] each, NULL = not wanted
     type(c_ptr) :: dbz, vd, sw, vz_r, vz_s, vz_g, dbz_r, dbz_s, dbz_g
  end type kidmp_doppler_out
  type, bind(C) :: kidmp_lidar_out                       ! kidmp_lidar_out / kidmp32_lidar_out: [ncol][nz] each, NULL = not wanted
     type(c_ptr) :: ext_c, ext_i, ext_r, ext_s, ext_g, ext, bsc, bsc_mol, tau_up, tau_dn, att_up, att_dn, sr_up, sr_dn
  end type kidmp_lidar_out

  type, bind(C) :: kidmp_spectra_out                     ! kidmp_spectra_out / kidmp32_spectra_out: [ncol][nz] each, NULL = not wanted
     type(c_ptr) :: lam_c, n0_c, nu_c, lam_i, n0_i, lam_r, n0_r, smob, smoc, lam_g, n0_g
  end type kidmp_spectra_out
  type, bind(C) :: kidmp_spectra_bins                    ! kidmp_spectra_bins / kidmp32_spectra_bins: [ncol][nb][nz] each, NULL = not wanted
     type(c_ptr) :: n_c, n_i, n_r, n_s, n_g
  end type kidmp_spectra_bins
  type, bind(C) :: kidmp_spectra_grids                   ! by species c, i, r, s, g: D and dD both NULL = the scheme's own 100 bins
     type(c_ptr) :: D(5), dD(5)
     integer(c_int32_t) :: nb(5)
  end type kidmp_spectra_grids

  type, bind(C) :: kidmp_dspectrum_out                   ! kidmp_dspectrum_out / kidmp32_dspectrum_out: NULL = not wanted
     type(c_ptr) :: total, rain, snow, graupel, below, above
  end type kidmp_dspectrum_out
  type, bind(C) :: kidmp_dspectrum_grids                 ! by species r, s, g: D and dD both NULL = the scheme's own 100 bins
     type(c_ptr) :: D(3), dD(3)
     integer(c_int32_t) :: nb(3)
  end type kidmp_dspectrum_grids

  type, bind(C) :: kidmp_brightband_out                  ! kidmp_brightband_out / kidmp32_brightband_out: NULL = not wanted
     type(c_ptr) :: dbz, dbz_s, dbz_g, enh_s, enh_g, fmelt_s, fmelt_g, k0
  end type kidmp_brightband_out
  type, bind(C) :: kidmp_brightband_grids                ! by species s, g: D and dD both NULL = the scheme's own 100 bins
     type(c_ptr) :: D(2), dD(2)
     integer(c_int32_t) :: nb(2)
  end type kidmp_brightband_grids
  type, bind(C) :: kidmp_brightband_cfg                  ! kidmp_brightband_cfg; kidmp_brightband_defaults fills it
     real(c_double) :: eps_w_re, eps_w_im, eps_i, rho_w, rho_i, kw2
     integer(c_int32_t) :: topology
  end type kidmp_brightband_cfg

  type, bind(C) :: kidmp_mie_out                         ! kidmp_mie_out / kidmp32_mie_out: NULL = not wanted
     type(c_ptr) :: dbz, dbz_up, dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, mie_g, ext, pia_up, pia_down, vd, pia_total
  end type kidmp_mie_out
  type, bind(C) :: kidmp_mie_cfg                         ! kidmp_mie_cfg; kidmp_mie_defaults fills it
     real(c_double) :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, rho_w, rho_i, kw2
  end type kidmp_mie_cfg
  type, bind(C) :: kidmp_pol_out                         ! kidmp_pol_out / kidmp32_pol_out: NULL = not wanted
     type(c_ptr) :: dbz_h, zdr, kdp, rhohv, dbz_h_r, dbz_h_s, dbz_h_g, zdr_r, zdr_s, zdr_g, kdp_r, kdp_s, kdp_g
  end type kidmp_pol_out
  type, bind(C) :: kidmp_pol_cfg                         ! kidmp_pol_cfg; kidmp_pol_defaults fills it
     real(c_double) :: axis_r(5), axis_r_min, axis_s, axis_g, sigma(3)
     integer(c_int32_t) :: force_quadrature
  end type kidmp_pol_cfg
  type, bind(C) :: kidmp_radiometer_out                  ! kidmp_radiometer_out / kidmp32_radiometer_out: NULL = not wanted
     type(c_ptr) :: k_abs, k_bsc, refl, trans, tb_up, tb_down, tb_toa, tb_ground, tau_abs
  end type kidmp_radiometer_out
  type, bind(C) :: kidmp_radiometer_cfg                  ! kidmp_radiometer_cfg; kidmp_radiometer_defaults fills it
     real(c_double) :: mu, emissivity, t_cosmic
  end type kidmp_radiometer_cfg

  type, bind(C) :: kidmp_kid_fields                      ! kidmp_kid_fields / kidmp32_kid_fields: KiD's fields, [ncol][nz] each
     type(c_ptr) :: theta, qv, qc, qr, nr, qi, ni, qs, qg
  end type kidmp_kid_fields

  type(c_ptr), save :: ctx = c_null_ptr                  ! the context (of the first device, when there are several)
  type(c_ptr), save :: mctx = c_null_ptr                 ! kidmp_multi handle, when kidmp_ndevices > 1
  ! Staging arrays of mp_thompson_batch: page-locked (kidmp_host_alloc) and kept between calls, so that the library's
  ! upload / step / download pipeline can move them by DMA.  1 = state (12 profiles), 2 = p, w, dz, 3 = ppt,
  ! 4 = the 36 rate profiles, 5 = the substep counts, 6 = the column outputs dbz, re_qc, re_qi, re_qs (only when asked for).
  ! 7 = the hydrometeor moments of mp_thompson_kid_interface (mp_thompson_kid_staging).
  type(c_ptr), save :: hbuf(7) = c_null_ptr
  integer(c_size_t), save :: hbytes(7) = 0_c_size_t

  interface
     integer(c_int) function kidmp_init(cfg, ctx_out) bind(C, name='kidmp_init')
       import :: c_int, c_ptr, kidmp_cfg
       type(kidmp_cfg), intent(in) :: cfg
       type(c_ptr), intent(out) :: ctx_out
     end function kidmp_init
     subroutine kidmp_finalize(ctx) bind(C, name='kidmp_finalize')
       import :: c_ptr
       type(c_ptr), value :: ctx
     end subroutine kidmp_finalize
     function kidmp_last_error(ctx) result(msg) bind(C, name='kidmp_last_error')
       import :: c_ptr
       type(c_ptr), value :: ctx
       type(c_ptr) :: msg
     end function kidmp_last_error
     integer(c_int) function kidmp_init_multi(cfg, ndev, devices, m_out) bind(C, name='kidmp_init_multi')
       import :: c_int, c_int32_t, c_ptr, kidmp_cfg
       type(kidmp_cfg), intent(in) :: cfg
       integer(c_int32_t), value :: ndev
       integer(c_int32_t), intent(in) :: devices(*)
       type(c_ptr), intent(out) :: m_out
     end function kidmp_init_multi
     subroutine kidmp_finalize_multi(m) bind(C, name='kidmp_finalize_multi')
       import :: c_ptr
       type(c_ptr), value :: m
     end subroutine kidmp_finalize_multi
     type(c_ptr) function kidmp_multi_context(m, i) bind(C, name='kidmp_multi_context')
       import :: c_ptr, c_int32_t
       type(c_ptr), value :: m
       integer(c_int32_t), value :: i
     end function kidmp_multi_context
     function kidmp_multi_last_error(m) result(msg) bind(C, name='kidmp_multi_last_error')
       import :: c_ptr
       type(c_ptr), value :: m
       type(c_ptr) :: msg
     end function kidmp_multi_last_error
     integer(c_int) function kidmp_batch_step_host_multi(m, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, &
          nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, precip_sums) bind(C, name='kidmp_batch_step_host_multi')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value :: m
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       real(c_double), value :: dt
       type(c_ptr), value :: qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep
       real(c_double), intent(out) :: precip_sums(4)
     end function kidmp_batch_step_host_multi
     integer(c_int) function kidmp_table_cache_reuse(ctx, dir, l_reuse, write_if_built, status) &
          bind(C, name='kidmp_table_cache_reuse')
       import :: c_int, c_int32_t, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: dir(*)
       integer(c_int32_t), value :: l_reuse, write_if_built
       integer(c_int32_t), intent(out) :: status
     end function kidmp_table_cache_reuse
     integer(c_int) function kidmp_set_column_nc(ctx, ncol, set_nc) bind(C, name='kidmp_set_column_nc')
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       type(c_ptr), value :: set_nc
     end function kidmp_set_column_nc
     type(c_ptr) function kidmp_host_alloc(bytes) bind(C, name='kidmp_host_alloc')   ! page-locked host memory
       import :: c_ptr, c_size_t
       integer(c_size_t), value :: bytes
     end function kidmp_host_alloc
     subroutine kidmp_host_free(p) bind(C, name='kidmp_host_free')
       import :: c_ptr
       type(c_ptr), value :: p
     end subroutine kidmp_host_free
     ! calc_refl10cm, M:4946-5244 (include/kidmp.h): t, p, qv, qr, nr, qs, qg in, dbz out; qs/qg NULL in a warm run
     integer(c_int) function kidmp_reflectivity_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz) &
          bind(C, name='kidmp_reflectivity_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, dbz         ! real(c_double) [ncol][nz]
     end function kidmp_reflectivity_host
     integer(c_int) function kidmp32_reflectivity_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz) &
          bind(C, name='kidmp32_reflectivity_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, dbz         ! real(c_float) [ncol][nz]
     end function kidmp32_reflectivity_host
     ! calc_effectRad, M:4834-4935 (include/kidmp.h): n = ncol*nz elements; re_* INOUT; nc, qi + ni, qs may be NULL
     integer(c_int) function kidmp_effective_radii_host(ctx, n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs) &
          bind(C, name='kidmp_effective_radii_host')
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: n
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs   ! real(c_double) [n]
     end function kidmp_effective_radii_host
     integer(c_int) function kidmp32_effective_radii_host(ctx, n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs) &
          bind(C, name='kidmp32_effective_radii_host')
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: n
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs   ! real(c_float) [n]
     end function kidmp32_effective_radii_host
     ! the step followed by the outputs of the post-step state (nothing requested in `out`: the plain step).  Arrays by
     ! address: the ones KiD never fills (nc, nwfa, nifa, w; the frozen species of a warm run) may be NULL
     integer(c_int) function kidmp_batch_step_host_out(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, &
          nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, out) bind(C, name='kidmp_batch_step_host_out')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_outputs
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       real(c_double), value :: dt
       type(c_ptr), value :: qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt
       type(c_ptr), value :: rates, nstep
       type(kidmp_outputs), intent(in) :: out
     end function kidmp_batch_step_host_out
     integer(c_int) function kidmp32_batch_step_host_out(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, &
          nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, arith, out) bind(C, name='kidmp32_batch_step_host_out')
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr, kidmp_outputs
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz, arith
       real(c_float), value :: dt
       type(c_ptr), value :: qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt
       type(c_ptr), value :: rates, nstep
       type(kidmp_outputs), intent(in) :: out
     end function kidmp32_batch_step_host_out
     ! mphys_thompson09_interfacen (W:28-310) on host arrays: gather, step, outputs and back-out on the GPU
     integer(c_int) function kidmp_kid_interface_host(ctx, ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, &
          ppt, rates, nstep, out) bind(C, name='kidmp_kid_interface_host')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_outputs, kidmp_kid_fields
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       real(c_double), value :: dt, p0, r_on_cp
       type(kidmp_kid_fields), intent(in) :: state, adv, div, mphys
       type(c_ptr), value :: exner, dz, ppt, rates, nstep
       type(kidmp_outputs), intent(in) :: out
     end function kidmp_kid_interface_host
     integer(c_int) function kidmp32_kid_interface_host(ctx, ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, &
          ppt, rates, nstep, out, arith) bind(C, name='kidmp32_kid_interface_host')
       import :: c_int, c_int32_t, c_int64_t, c_float, c_ptr, kidmp_outputs, kidmp_kid_fields
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz, arith
       real(c_float), value :: dt, p0, r_on_cp
       type(kidmp_kid_fields), intent(in) :: state, adv, div, mphys
       type(c_ptr), value :: exner, dz, ppt, rates, nstep
       type(kidmp_outputs), intent(in) :: out
     end function kidmp32_kid_interface_host
     ! the per-column summary (include/kidmp_summary.h): summary [ncol][16] is real(c_double) in both; nc, qi, qs + qg and
     ! cfg may be NULL; dz_col_stride 0 = one dz profile for all columns
     integer(c_int) function kidmp_column_summary_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, qr, nr, qs, qg, dz, &
          dz_col_stride, cfg, summary) bind(C, name='kidmp_column_summary_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, qr, nr, qs, qg, dz   ! real(c_double) [ncol][nz], dz [nz]
       type(c_ptr), value :: cfg, summary
     end function kidmp_column_summary_host
     integer(c_int) function kidmp32_column_summary_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, qr, nr, qs, qg, dz, &
          dz_col_stride, cfg, summary) bind(C, name='kidmp32_column_summary_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, qr, nr, qs, qg, dz   ! real(c_float) [ncol][nz], dz [nz]
       type(c_ptr), value :: cfg, summary
     end function kidmp32_column_summary_host
     ! block-O fall speeds and sedimentation fluxes (include/kidmp_fall.h): qi, ni, qs, qg, vts_boost may be NULL as the
     ! header says; dz, dz_col_stride and dt are read only when nstep is not NULL; nstep [ncol][4] int32
     integer(c_int) function kidmp_fall_speeds_host(ctx, ncol, nz, t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, &
          dz_col_stride, dt, out, nstep) bind(C, name='kidmp_fall_speeds_host')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_fall_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz   ! real(c_double) [ncol][nz], dz [nz]
       real(c_double), value :: dt
       type(kidmp_fall_out), intent(in) :: out
       type(c_ptr), value :: nstep
     end function kidmp_fall_speeds_host
     integer(c_int) function kidmp32_fall_speeds_host(ctx, ncol, nz, t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, &
          dz_col_stride, dt, out, nstep) bind(C, name='kidmp32_fall_speeds_host')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_fall_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz   ! real(c_float) [ncol][nz], dz [nz]
       real(c_double), value :: dt
       type(kidmp_fall_out), intent(in) :: out
       type(c_ptr), value :: nstep
     end function kidmp32_fall_speeds_host
     ! the size spectra (include/kidmp_spectra.h): nc, qi, ni, qs, qg may be NULL as the header says
     integer(c_int) function kidmp_size_spectra_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids) &
          bind(C, name='kidmp_size_spectra_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_spectra_out, kidmp_spectra_bins, kidmp_spectra_grids
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg   ! real(c_double) [ncol][nz]
       type(kidmp_spectra_out), intent(in) :: par
       type(kidmp_spectra_bins), intent(in) :: bins
       type(kidmp_spectra_grids), intent(in) :: grids
     end function kidmp_size_spectra_host
     integer(c_int) function kidmp32_size_spectra_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids) &
          bind(C, name='kidmp32_size_spectra_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_spectra_out, kidmp_spectra_bins, kidmp_spectra_grids
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg   ! real(c_float) [ncol][nz]
       type(kidmp_spectra_out), intent(in) :: par
       type(kidmp_spectra_bins), intent(in) :: bins
       type(kidmp_spectra_grids), intent(in) :: grids
     end function kidmp32_size_spectra_host
     ! the Doppler moments of a vertically pointing radar (include/kidmp_doppler.h): qs, qg and w may be NULL (zero)
     integer(c_int) function kidmp_doppler_moments_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, w, out) &
          bind(C, name='kidmp_doppler_moments_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_doppler_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, w   ! real(c_double) [ncol][nz]
       type(kidmp_doppler_out), intent(in) :: out
     end function kidmp_doppler_moments_host
     integer(c_int) function kidmp32_doppler_moments_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, w, out) &
          bind(C, name='kidmp32_doppler_moments_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_doppler_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, w   ! real(c_float) [ncol][nz]
       type(kidmp_doppler_out), intent(in) :: out
     end function kidmp32_doppler_moments_host
     ! the lidar operator (include/kidmp_lidar.h): nc, qi, ni, qs, qg, cfg (nine doubles) and summary [ncol][8] (real(c_double)
     ! in both) may be NULL; dz_col_stride 0 = one dz profile for all columns
     integer(c_int) function kidmp_lidar_profiles_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, &
          dz_col_stride, cfg, out, summary) bind(C, name='kidmp_lidar_profiles_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_lidar_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz   ! real(c_double) [ncol][nz], dz [nz]
       type(c_ptr), value :: cfg, summary
       type(kidmp_lidar_out), intent(in) :: out
     end function kidmp_lidar_profiles_host
     integer(c_int) function kidmp32_lidar_profiles_host(ctx, ncol, nz, t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, &
          dz_col_stride, cfg, out, summary) bind(C, name='kidmp32_lidar_profiles_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_lidar_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol, dz_col_stride
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz   ! real(c_float) [ncol][nz], dz [nz]
       type(c_ptr), value :: cfg, summary
       type(kidmp_lidar_out), intent(in) :: out
     end function kidmp32_lidar_profiles_host
     ! the Doppler spectrum on a uniform velocity grid (include/kidmp_dspectrum.h): qs, qg and w may be NULL (zero)
     integer(c_int) function kidmp_doppler_spectrum_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out) &
          bind(C, name='kidmp_doppler_spectrum_host')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_dspectrum_grids, kidmp_dspectrum_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz, nv
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, w
       real(c_double), value :: v0, dv
       type(kidmp_dspectrum_grids), intent(in) :: grids
       type(kidmp_dspectrum_out), intent(in) :: out
     end function kidmp_doppler_spectrum_host
     integer(c_int) function kidmp32_doppler_spectrum_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out) &
          bind(C, name='kidmp32_doppler_spectrum_host')
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr, kidmp_dspectrum_grids, kidmp_dspectrum_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz, nv
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, w
       real(c_double), value :: v0, dv
       type(kidmp_dspectrum_grids), intent(in) :: grids
       type(kidmp_dspectrum_out), intent(in) :: out
     end function kidmp32_doppler_spectrum_host
     ! the reflectivity with its melting layer (include/kidmp_brightband.h): qs and qg may be NULL (zero), cfg NULL = defaults
     subroutine kidmp_brightband_defaults(cfg) bind(C, name='kidmp_brightband_defaults')
       import :: kidmp_brightband_cfg
       type(kidmp_brightband_cfg), intent(out) :: cfg
     end subroutine kidmp_brightband_defaults
     integer(c_int) function kidmp_bright_band_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, cfg, grids, out) &
          bind(C, name='kidmp_bright_band_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_brightband_grids, kidmp_brightband_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, cfg
       type(kidmp_brightband_grids), intent(in) :: grids
       type(kidmp_brightband_out), intent(in) :: out
     end function kidmp_bright_band_host
     integer(c_int) function kidmp32_bright_band_host(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, cfg, grids, out) &
          bind(C, name='kidmp32_bright_band_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_brightband_grids, kidmp_brightband_out
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg, cfg
       type(kidmp_brightband_grids), intent(in) :: grids
       type(kidmp_brightband_out), intent(in) :: out
     end function kidmp32_bright_band_host
     ! the cloud radar (include/kidmp_mie.h): a table of Mie rows per wavelength, then the operator; qc, qs, qg, dz, w and
     ! k_gas may be NULL
     subroutine kidmp_mie_defaults(cfg) bind(C, name='kidmp_mie_defaults')
       import :: kidmp_mie_cfg
       type(kidmp_mie_cfg), intent(out) :: cfg
     end subroutine kidmp_mie_defaults
     integer(c_int) function kidmp_mie_table_create(ctx, cfg, grids, table) bind(C, name='kidmp_mie_table_create')
       import :: c_int, c_ptr, kidmp_mie_cfg
       type(c_ptr), value :: ctx, grids
       type(kidmp_mie_cfg), intent(in) :: cfg
       type(c_ptr), intent(out) :: table
     end function kidmp_mie_table_create
     subroutine kidmp_mie_table_destroy(table) bind(C, name='kidmp_mie_table_destroy')
       import :: c_ptr
       type(c_ptr), value :: table
     end subroutine kidmp_mie_table_destroy
     integer(c_int) function kidmp_mie_radar_host(ctx, table, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, &
          k_gas, k_gas_col_stride, out) bind(C, name='kidmp_mie_radar_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_mie_out
       type(c_ptr), value :: ctx, table
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: w, k_gas
       integer(c_int64_t), value :: k_gas_col_stride
       type(kidmp_mie_out), intent(in) :: out
     end function kidmp_mie_radar_host
     integer(c_int) function kidmp32_mie_radar_host(ctx, table, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, &
          k_gas, k_gas_col_stride, out) bind(C, name='kidmp32_mie_radar_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_mie_out
       type(c_ptr), value :: ctx, table
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: w, k_gas
       integer(c_int64_t), value :: k_gas_col_stride
       type(kidmp_mie_out), intent(in) :: out
     end function kidmp32_mie_radar_host
     ! the radiometer (include/kidmp_radiometer.h): a table of three rows per bin and wavelength, then the operator; qc, qs,
     ! qg, k_gas and t_sfc may be NULL
     subroutine kidmp_radiometer_defaults(rcfg) bind(C, name='kidmp_radiometer_defaults')
       import :: kidmp_radiometer_cfg
       type(kidmp_radiometer_cfg), intent(out) :: rcfg
     end subroutine kidmp_radiometer_defaults
     integer(c_int) function kidmp_radiometer_table_create(ctx, cfg, grids, table) bind(C, name='kidmp_radiometer_table_create')
       import :: c_int, c_ptr, kidmp_mie_cfg
       type(c_ptr), value :: ctx, grids
       type(kidmp_mie_cfg), intent(in) :: cfg
       type(c_ptr), intent(out) :: table
     end function kidmp_radiometer_table_create
     subroutine kidmp_radiometer_table_destroy(table) bind(C, name='kidmp_radiometer_table_destroy')
       import :: c_ptr
       type(c_ptr), value :: table
     end subroutine kidmp_radiometer_table_destroy
     integer(c_int) function kidmp_radiometer_host(ctx, table, rcfg, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, &
          k_gas_col_stride, t_sfc, out) bind(C, name='kidmp_radiometer_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_radiometer_cfg, kidmp_radiometer_out
       type(c_ptr), value :: ctx, table
       type(kidmp_radiometer_cfg), intent(in) :: rcfg
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: k_gas
       integer(c_int64_t), value :: k_gas_col_stride
       type(c_ptr), value :: t_sfc
       type(kidmp_radiometer_out), intent(in) :: out
     end function kidmp_radiometer_host
     integer(c_int) function kidmp32_radiometer_host(ctx, table, rcfg, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, &
          k_gas_col_stride, t_sfc, out) bind(C, name='kidmp32_radiometer_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_radiometer_cfg, kidmp_radiometer_out
       type(c_ptr), value :: ctx, table
       type(kidmp_radiometer_cfg), intent(in) :: rcfg
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: k_gas
       integer(c_int64_t), value :: k_gas_col_stride
       type(c_ptr), value :: t_sfc
       type(kidmp_radiometer_out), intent(in) :: out
     end function kidmp32_radiometer_host
     ! several channels in one launch (include/kidmp_multichannel.h): tables is an array of nch handles, rcfg one of nch
     ! closures, the outputs carry a leading (in C) channel dimension
     integer(c_int) function kidmp_radiometer_multi_host(ctx, tables, nch, rcfg, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, &
          dz_col_stride, k_gas, k_gas_col_stride, k_gas_ch_stride, t_sfc, out) bind(C, name='kidmp_radiometer_multi_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_radiometer_cfg, kidmp_radiometer_out
       type(c_ptr), value :: ctx
       type(c_ptr), intent(in) :: tables(*)
       integer(c_int32_t), value :: nch
       type(kidmp_radiometer_cfg), intent(in) :: rcfg(*)
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: k_gas
       integer(c_int64_t), value :: k_gas_col_stride, k_gas_ch_stride
       type(c_ptr), value :: t_sfc
       type(kidmp_radiometer_out), intent(in) :: out
     end function kidmp_radiometer_multi_host
     integer(c_int) function kidmp32_radiometer_multi_host(ctx, tables, nch, rcfg, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, &
          dz_col_stride, k_gas, k_gas_col_stride, k_gas_ch_stride, t_sfc, out) bind(C, name='kidmp32_radiometer_multi_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_radiometer_cfg, kidmp_radiometer_out
       type(c_ptr), value :: ctx
       type(c_ptr), intent(in) :: tables(*)
       integer(c_int32_t), value :: nch
       type(kidmp_radiometer_cfg), intent(in) :: rcfg(*)
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: k_gas
       integer(c_int64_t), value :: k_gas_col_stride, k_gas_ch_stride
       type(c_ptr), value :: t_sfc
       type(kidmp_radiometer_out), intent(in) :: out
     end function kidmp32_radiometer_multi_host
     integer(c_int) function kidmp_mie_radar_multi_host(ctx, tables, nch, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, &
          w, k_gas, k_gas_col_stride, k_gas_ch_stride, out) bind(C, name='kidmp_mie_radar_multi_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_mie_out
       type(c_ptr), value :: ctx
       type(c_ptr), intent(in) :: tables(*)
       integer(c_int32_t), value :: nch
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: w, k_gas
       integer(c_int64_t), value :: k_gas_col_stride, k_gas_ch_stride
       type(kidmp_mie_out), intent(in) :: out
     end function kidmp_mie_radar_multi_host
     integer(c_int) function kidmp32_mie_radar_multi_host(ctx, tables, nch, ncol, nz, t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, &
          w, k_gas, k_gas_col_stride, k_gas_ch_stride, out) bind(C, name='kidmp32_mie_radar_multi_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_mie_out
       type(c_ptr), value :: ctx
       type(c_ptr), intent(in) :: tables(*)
       integer(c_int32_t), value :: nch
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qc, qr, nr, qs, qg, dz
       integer(c_int64_t), value :: dz_col_stride
       type(c_ptr), value :: w, k_gas
       integer(c_int64_t), value :: k_gas_col_stride, k_gas_ch_stride
       type(kidmp_mie_out), intent(in) :: out
     end function kidmp32_mie_radar_multi_host
     ! the polarimetric radar (include/kidmp_polarimetric.h): a table of seven rows per bin, then the operator; qs and qg
     ! may be NULL
     subroutine kidmp_pol_defaults(pcfg) bind(C, name='kidmp_pol_defaults')
       import :: kidmp_pol_cfg
       type(kidmp_pol_cfg), intent(out) :: pcfg
     end subroutine kidmp_pol_defaults
     integer(c_int) function kidmp_pol_table_create(ctx, cfg, pcfg, grids, table) bind(C, name='kidmp_pol_table_create')
       import :: c_int, c_ptr, kidmp_mie_cfg, kidmp_pol_cfg
       type(c_ptr), value :: ctx
       type(kidmp_mie_cfg), intent(in) :: cfg
       type(kidmp_pol_cfg), intent(in) :: pcfg
       type(c_ptr), value :: grids
       type(c_ptr), intent(out) :: table
     end function kidmp_pol_table_create
     subroutine kidmp_pol_table_destroy(table) bind(C, name='kidmp_pol_table_destroy')
       import :: c_ptr
       type(c_ptr), value :: table
     end subroutine kidmp_pol_table_destroy
     integer(c_int) function kidmp_polarimetric_host(ctx, table, ncol, nz, t, p, qv, qr, nr, qs, qg, out) &
          bind(C, name='kidmp_polarimetric_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_pol_out
       type(c_ptr), value :: ctx, table
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg
       type(kidmp_pol_out), intent(in) :: out
     end function kidmp_polarimetric_host
     integer(c_int) function kidmp32_polarimetric_host(ctx, table, ncol, nz, t, p, qv, qr, nr, qs, qg, out) &
          bind(C, name='kidmp32_polarimetric_host')
       import :: c_int, c_int32_t, c_int64_t, c_ptr, kidmp_pol_out
       type(c_ptr), value :: ctx, table
       integer(c_int64_t), value :: ncol
       integer(c_int32_t), value :: nz
       type(c_ptr), value :: t, p, qv, qr, nr, qs, qg
       type(kidmp_pol_out), intent(in) :: out
     end function kidmp32_polarimetric_host
  end interface

contains

  ! .true. when mp_thompson_batch ran on several devices and kidmp_precip_sums holds the RCCL-reduced domain sums
  logical function kidmp_precip_sums_valid()
    kidmp_precip_sums_valid = c_associated(mctx)
  end function kidmp_precip_sums_valid

  subroutine stop_on_error(rc, where)
    integer(c_int), intent(in) :: rc
    character(*), intent(in) :: where
    character(kind=c_char), pointer :: cmsg(:)
    type(c_ptr) :: p
    integer :: n
    if (rc == 0) return
    if (c_associated(mctx)) then
       p = kidmp_multi_last_error(mctx)
    else
       p = kidmp_last_error(ctx)
    end if
    write(*,'(a,a,a,i0)') ' module_mp_thompson09n: ', where, ' failed, kidmp code ', rc
    if (c_associated(p)) then
       call c_f_pointer(p, cmsg, [512])
       n = 1
       do while (n < 512 .and. cmsg(n) /= c_null_char)
          n = n + 1
       end do
       write(*,'(1x,512a1)') cmsg(1:n-1)
    end if
    stop 1      ! the reference aborts on init failure too (Fortran runtime error at M:3718)
  end subroutine stop_on_error

  ! hbuf(i) with room for `need` bytes (grown, never shrunk)
  subroutine staging(i, need)
    integer, intent(in) :: i
    integer(c_size_t), intent(in) :: need
    if (need <= hbytes(i) .and. c_associated(hbuf(i))) return
    if (c_associated(hbuf(i))) call kidmp_host_free(hbuf(i))
    hbuf(i) = kidmp_host_alloc(need)
    hbytes(i) = need
    if (.not. c_associated(hbuf(i))) then
       write(*,'(a,i0,a)') ' module_mp_thompson09n: kidmp_host_alloc(', need, ') failed'
       stop 1
    end if
  end subroutine staging

  ! the address `off` bytes into the block at p
  type(c_ptr) function byte_offset(p, off)
    type(c_ptr), intent(in) :: p
    integer(c_size_t), intent(in) :: off
    integer(c_int8_t), pointer :: b(:)
    call c_f_pointer(p, b, [off + 1])
    byte_offset = c_loc(b(off + 1))
  end function byte_offset

  ! the `arith` argument of the kidmp32_* entries (KIDMP_ARITH_P32N, KIDMP_ARITH_F32)
  integer(c_int32_t) function arith_code()
    arith_code = merge(1_c_int32_t, 0_c_int32_t, trim(kidmp_arith) == 'f32')
  end function arith_code

  subroutine radii_together(have_qc, have_qi, have_qs)
    logical, intent(in) :: have_qc, have_qi, have_qs
    if ((have_qc .neqv. have_qi) .or. (have_qc .neqv. have_qs)) then
       write(*,'(a)') ' module_mp_thompson09n: re_qc, re_qi, re_qs must be passed or left out together'
       stop 1
    end if
  end subroutine radii_together

  ! With l_rate_diagnostics the page-locked arrays the step writes its rates and substep counts to, in the C ABI's layout
  ! [ncol][36][nz] / [ncol][4], and their addresses; else NULL: nothing is diagnosed.
  subroutine rate_staging(ncol, nz, rates, nstep, prates, pnstep)
    integer, intent(in) :: ncol, nz
    real(c_double), pointer, intent(out) :: rates(:,:,:)
    integer(c_int32_t), pointer, intent(out) :: nstep(:,:)
    type(c_ptr), intent(out) :: prates, pnstep
    nullify(rates, nstep)
    prates = c_null_ptr;  pnstep = c_null_ptr
    if (.not. l_rate_diagnostics) return
    call staging(4, 8_c_size_t * NRATES * int(nz, c_size_t) * int(ncol, c_size_t))
    call staging(5, 16_c_size_t * ncol)
    call c_f_pointer(hbuf(4), rates, [nz, NRATES, ncol])
    call c_f_pointer(hbuf(5), nstep, [4, ncol])
    prates = hbuf(4);  pnstep = hbuf(5)
  end subroutine rate_staging

  ! one kidmp_kid_fields: theta-like, qv-like and the seven moments of hyd(nz*ncol, 7)
  function kid_fields(n, th, qv, hyd) result(f)
    integer, intent(in) :: n
    real, intent(in), target :: th(n), qv(n), hyd(n, 7)
    type(kidmp_kid_fields) :: f
    f = kidmp_kid_fields(c_loc(th), c_loc(qv), c_loc(hyd(1,1)), c_loc(hyd(1,2)), c_loc(hyd(1,3)), c_loc(hyd(1,4)), &
         c_loc(hyd(1,5)), c_loc(hyd(1,6)), c_loc(hyd(1,7)))
  end function kid_fields

  ! thompson_init, M:374-797: constants on the host, lookup tables built on the GPU (on every GPU of the device list).
  subroutine thompson_init
    type(kidmp_cfg) :: cfg
    integer(c_int) :: rc
    integer(c_int32_t) :: devs(8), status, reuse, wr
    type(c_ptr) :: c
    character(64) :: envdev
    character(kind=c_char) :: cdir(65)
    integer :: envstat, i, n, pos, nxt
    if (c_associated(ctx)) return                         ! micro_init guard, M:384-389
    cfg%iiwarm = merge(1_c_int32_t, 0_c_int32_t, iiwarm)
    cfg%l_sediment = merge(1_c_int32_t, 0_c_int32_t, l_sediment)
    cfg%set_Nc = real(set_Nc, c_double)
    call get_environment_variable('KIDMP_DEVICE', envdev, status=envstat)
    if (envstat == 0 .and. len_trim(envdev) > 0) read(envdev, *, iostat=envstat) kidmp_device
    call get_environment_variable('KIDMP_DEVICES', envdev, status=envstat)    ! "0,1,2,3": several GPUs
    if (envstat == 0 .and. len_trim(envdev) > 0) then
       n = 0;  pos = 1
       do while (pos <= len_trim(envdev) .and. n < 8)
          nxt = index(envdev(pos:), ',')
          if (nxt == 0) nxt = len_trim(envdev) - pos + 2
          n = n + 1
          read(envdev(pos:pos+nxt-2), *, iostat=envstat) kidmp_devices(n)
          if (envstat /= 0) then
             write(*,'(2a)') ' module_mp_thompson09n: cannot read KIDMP_DEVICES=', trim(envdev)
             stop 1
          end if
          pos = pos + nxt
       end do
       kidmp_ndevices = n
       ! a list with ONE entry names the card of the single-device path (KIDMP_DEVICES=3 must not land on GPU 0)
       if (n == 1) kidmp_device = kidmp_devices(1)
    end if
    cfg%device = int(kidmp_device, c_int32_t)
    cfg%is_aerosol_aware = merge(1_c_int32_t, 0_c_int32_t, is_aerosol_aware)
    if (kidmp_ndevices > 1) then
       if (kidmp_ndevices > 8) then
          write(*,'(a)') ' module_mp_thompson09n: at most 8 devices'
          stop 1
       end if
       if (trim(kidmp_arith) /= 'p64') then
          write(*,'(a)') ' module_mp_thompson09n: several devices need kidmp_arith = p64'
          stop 1
       end if
       devs(1:kidmp_ndevices) = int(kidmp_devices(1:kidmp_ndevices), c_int32_t)
       rc = kidmp_init_multi(cfg, int(kidmp_ndevices, c_int32_t), devs, mctx)
       call stop_on_error(rc, 'thompson_init (kidmp_init_multi)')
       ctx = kidmp_multi_context(mctx, 0_c_int32_t)
    else
       rc = kidmp_init(cfg, ctx)
       call stop_on_error(rc, 'thompson_init')
    end if
    ! ---- the reference's table cache, M:3717-3729 / M:3822-3829 and M:3864-3895 / M:4065-4078: per file, read it if
    !      it exists and l_reuse_thompson_lookup is set, else write the freshly built tables (first device only) ----
    if (.not. iiwarm) then
       n = len_trim(kidmp_cache_dir)
       do i = 1, n
          cdir(i) = kidmp_cache_dir(i:i)
       end do
       cdir(n+1) = c_null_char
       reuse = merge(1_c_int32_t, 0_c_int32_t, l_reuse_thompson_lookup)
       do i = 1, max(1, kidmp_ndevices)
          c = ctx
          if (c_associated(mctx)) c = kidmp_multi_context(mctx, int(i-1, c_int32_t))
          wr = merge(1_c_int32_t, 0_c_int32_t, i == 1)
          rc = kidmp_table_cache_reuse(c, cdir, reuse, wr, status)
          call stop_on_error(rc, 'thompson_init (table cache)')
          if (i == 1 .and. iand(status, 2_c_int32_t) /= 0) then          ! the reference's notice: printed by qr_acr_qs only
             ! (M:3872-3881; qr_acr_qg reads its file silently, M:3721-3727), i.e. when the racs file was read (bit 1)
             write(6,*) ' !!!!!!!!!!!!!!!!!! WARNING !!!!!!!!!!!!!!!!!!!'
             write(6,*) ' Reading in pre-calculated lookup tables in    '
             write(6,*) ' Thompson scheme'
             write(6,*) ' If you have changed any microphysical '
             write(6,*) ' parameters, you may need to recalculate these. '
             write(6,*) ' !!!!!!!!!!!!!!!!!! WARNING !!!!!!!!!!!!!!!!!!!'
          end if
       end do
    end if
  end subroutine thompson_init

  subroutine thompson_finalize
    integer :: i
    do i = 1, size(hbuf)
       if (c_associated(hbuf(i))) call kidmp_host_free(hbuf(i))
       hbuf(i) = c_null_ptr;  hbytes(i) = 0_c_size_t
    end do
    if (c_associated(mctx)) then
       call kidmp_finalize_multi(mctx)                    ! finalises every context, ctx among them
    else if (c_associated(ctx)) then
       call kidmp_finalize(ctx)
    end if
    ctx = c_null_ptr;  mctx = c_null_ptr
  end subroutine thompson_finalize

  ! mp_thompson, M:1156-1177: one column, reference dummy list.
  subroutine mp_thompson (qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, &
       nr1d, nc1d, nwfa1d, nifa1d, t1d, p1d, w1d, dzq, &
       pptrain, pptsnow, pptgraul, pptice, &
       kts, kte, dt, ii, jj)
    integer, intent(in) :: kts, kte, ii, jj
    real, dimension(kts:kte), intent(inout) :: qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, &
         nr1d, nc1d, nwfa1d, nifa1d, t1d
    real, dimension(kts:kte), intent(in) :: p1d, w1d, dzq
    real, intent(inout) :: pptrain, pptsnow, pptgraul, pptice
    real, intent(in) :: dt
    real :: ppt(4,1)
    integer :: nz
    nz = kte - kts + 1
    ppt(:,1) = (/ pptrain, pptsnow, pptgraul, pptice /)
    call mp_thompson_batch(1, nz, dt, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, nc1d, nwfa1d, &
         nifa1d, t1d, p1d, w1d, dzq, ppt)
    pptrain = ppt(1,1); pptsnow = ppt(2,1); pptgraul = ppt(3,1); pptice = ppt(4,1)
    if (.false.) print *, ii, jj          ! ii, jj are debug-only in the reference (M:1269-1274)
  end subroutine mp_thompson

  ! calc_refl10cm, M:4946-5244, with the reference's dummy list: 10-cm radar reflectivity (dBZ) of one column.  qc1d is
  ! never read by the reference's live code and ii, jj only name the column: all three are accepted and ignored.  As
  ! shipped (nrbins = 0, M:204) there is no bright band.  Default REAL 8 goes to kidmp_reflectivity_host, REAL 4 to
  ! kidmp32_reflectivity_host (binary32 in and out, binary64 inside).
  subroutine calc_refl10cm (qv1d, qc1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d, dBZ, kts, kte, ii, jj)
    integer, intent(in) :: kts, kte, ii, jj
    real, dimension(kts:kte), intent(in) :: qv1d, qc1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d
    real, dimension(kts:kte), intent(inout) :: dBZ
    call calc_refl10cm_batch(1, kte - kts + 1, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d, dBZ)
    if (.false.) print *, qc1d(kts), ii, jj
  end subroutine calc_refl10cm

  ! calc_refl10cm over ncol columns of KiD's (nz, ncol) storage in one call.  qs, qg may be left out in an iiwarm run.
  subroutine calc_refl10cm_batch(ncol, nz, qv, qr, nr, qs, qg, t, p, dbz)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: qv, qr, nr, t, p
    real, dimension(nz,ncol), intent(in), optional, target :: qs, qg
    real, dimension(nz,ncol), intent(out), target :: dbz
    type(c_ptr) :: pqs, pqg
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    pqs = c_null_ptr;  pqg = c_null_ptr
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (kind(qv) == c_double) then
       rc = kidmp_reflectivity_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dbz))
    else
       rc = kidmp32_reflectivity_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dbz))
    end if
    call stop_on_error(rc, 'calc_refl10cm')
  end subroutine calc_refl10cm_batch

  ! calc_effectRad, M:4834-4935, with the reference's dummy list and intents: effective radii of cloud water, cloud ice
  ! and snow of one column; re_* are INOUT (a level without the species keeps the caller's value).  Default REAL 8 goes to
  ! kidmp_effective_radii_host, REAL 4 to kidmp32_effective_radii_host (binary32 in and out, binary64 inside).
  subroutine calc_effectRad (t1d, p1d, qv1d, qc1d, nc1d, qi1d, ni1d, qs1d, re_qc1d, re_qi1d, re_qs1d, kts, kte)
    integer, intent(in) :: kts, kte
    real, dimension(kts:kte), intent(in) :: t1d, p1d, qv1d, qc1d, nc1d, qi1d, ni1d, qs1d
    real, dimension(kts:kte), intent(inout) :: re_qc1d, re_qi1d, re_qs1d
    call calc_effectRad_batch(1, kte - kts + 1, t1d, p1d, qv1d, qc1d, re_qc1d, re_qi1d, re_qs1d, &
         nc=nc1d, qi=qi1d, ni=ni1d, qs=qs1d)
  end subroutine calc_effectRad

  ! calc_effectRad over ncol columns of KiD's (nz, ncol) storage in one call.  nc may be left out unless
  ! is_aerosol_aware (it is not read then, M:4863); qi, ni and qs in an iiwarm run (re_qi, re_qs then stay as they came).
  subroutine calc_effectRad_batch(ncol, nz, t, p, qv, qc, re_qc, re_qi, re_qs, nc, qi, ni, qs)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qc
    real, dimension(nz,ncol), intent(inout), target :: re_qc, re_qi, re_qs
    real, dimension(nz,ncol), intent(in), optional, target :: nc, qi, ni, qs
    type(c_ptr) :: pnc, pqi, pni, pqs
    integer(c_int64_t) :: n
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    pnc = c_null_ptr;  pqi = c_null_ptr;  pni = c_null_ptr;  pqs = c_null_ptr
    if (present(nc)) pnc = c_loc(nc)
    if (present(qi)) pqi = c_loc(qi)
    if (present(ni)) pni = c_loc(ni)
    if (present(qs)) pqs = c_loc(qs)
    n = int(ncol, c_int64_t) * int(nz, c_int64_t)
    if (kind(t) == c_double) then
       rc = kidmp_effective_radii_host(ctx, n, c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), pnc, pqi, pni, pqs, &
            c_loc(re_qc), c_loc(re_qi), c_loc(re_qs))
    else
       rc = kidmp32_effective_radii_host(ctx, n, c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), pnc, pqi, pni, pqs, &
            c_loc(re_qc), c_loc(re_qi), c_loc(re_qs))
    end if
    call stop_on_error(rc, 'calc_effectRad')
  end subroutine calc_effectRad_batch

  ! The per-column summary of include/kidmp_summary.h over ncol columns of KiD's (nz, ncol) storage in one call: water
  ! paths, liquid cloud optical depth, composite reflectivity, echo-top, cloud and freezing heights; summary(s+1, i) is slot
  ! s of column i, always real(c_double).  dz(nz) is KiD's one profile of layer depths.  nc may be left out unless
  ! is_aerosol_aware, qi, qs and qg in an iiwarm run; a threshold left out keeps the library's default (18 dBZ, 1e-5
  ! kg/kg, 273.15 K).  Default REAL 8 goes to kidmp_column_summary_host, REAL 4 to kidmp32_column_summary_host.
  subroutine column_summary_batch(ncol, nz, t, p, qv, qc, qr, nr, dz, summary, nc, qi, qs, qg, dbz_echo, q_cloud, t_freeze)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qc, qr, nr
    real, dimension(nz), intent(in), target :: dz
    real(c_double), dimension(16,ncol), intent(out), target :: summary
    real, dimension(nz,ncol), intent(in), optional, target :: nc, qi, qs, qg
    real, intent(in), optional :: dbz_echo, q_cloud, t_freeze
    real(c_double), target :: cfg(3)                       ! kidmp_summary_cfg: three doubles
    type(c_ptr) :: pnc, pqi, pqs, pqg, pcfg
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    pnc = c_null_ptr;  pqi = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pcfg = c_null_ptr
    if (present(nc)) pnc = c_loc(nc)
    if (present(qi)) pqi = c_loc(qi)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(dbz_echo) .or. present(q_cloud) .or. present(t_freeze)) then
       cfg = (/ 18.0_c_double, 1.0e-5_c_double, 273.15_c_double /)
       if (present(dbz_echo)) cfg(1) = real(dbz_echo, c_double)
       if (present(q_cloud)) cfg(2) = real(q_cloud, c_double)
       if (present(t_freeze)) cfg(3) = real(t_freeze, c_double)
       pcfg = c_loc(cfg)
    end if
    if (kind(t) == c_double) then
       rc = kidmp_column_summary_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qc), pnc, pqi, c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dz), 0_c_int64_t, pcfg, c_loc(summary))
    else
       rc = kidmp32_column_summary_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qc), pnc, pqi, c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dz), 0_c_int64_t, pcfg, c_loc(summary))
    end if
    call stop_on_error(rc, 'column_summary_batch')
  end subroutine column_summary_batch

  ! Block O (M:3206-3354) of a state over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_fall.h): the
  ! mass- and number-weighted fall speeds of rain, ice, snow and graupel (m s-1), the sedimentation fluxes v*rho*q per
  ! species and in total (kg m-2 s-1), and with dz(nz) and dt the substep counts nstep(4, ncol) (rain, ice, snow, graupel).
  ! Every output is optional, in the array kind the arithmetic stores; at least one must be present.  qi, ni, qs and qg
  ! may be left out in an iiwarm run; vts_boost left out means the value of a level without riming (1.0 below T_0, 1.5
  ! elsewhere).  The inputs are not changed.  Default REAL 8 goes to kidmp_fall_speeds_host, REAL 4 to kidmp32_...
  subroutine fall_speeds_batch(ncol, nz, t, p, qv, qr, nr, vt_r, vt_nr, vt_i, vt_ni, vt_s, vt_g, flux_r, flux_i, flux_s, &
       flux_g, flux_total, qi, ni, qs, qg, vts_boost, dz, dt, nstep)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: vt_r, vt_nr, vt_i, vt_ni, vt_s, vt_g, flux_r, flux_i, flux_s, &
         flux_g, flux_total
    real, dimension(nz,ncol), intent(in), optional, target :: qi, ni, qs, qg, vts_boost
    real, dimension(nz), intent(in), optional, target :: dz
    real, intent(in), optional :: dt
    integer(c_int32_t), dimension(4,ncol), intent(out), optional, target :: nstep
    type(kidmp_fall_out) :: out
    type(c_ptr) :: pqi, pni, pqs, pqg, pboost, pdz, pnstep
    real(c_double) :: dt8
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: fall speeds are not available with kidmp_ndevices > 1'
       stop 1
    end if
    pqi = c_null_ptr;  pni = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pboost = c_null_ptr
    pdz = c_null_ptr;  pnstep = c_null_ptr;  dt8 = 0.0_c_double
    if (present(qi)) pqi = c_loc(qi)
    if (present(ni)) pni = c_loc(ni)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(vts_boost)) pboost = c_loc(vts_boost)
    if (present(dz)) pdz = c_loc(dz)
    if (present(dt)) dt8 = real(dt, c_double)
    if (present(nstep)) pnstep = c_loc(nstep)
    out = kidmp_fall_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(vt_r)) out%vt_r = c_loc(vt_r)
    if (present(vt_nr)) out%vt_nr = c_loc(vt_nr)
    if (present(vt_i)) out%vt_i = c_loc(vt_i)
    if (present(vt_ni)) out%vt_ni = c_loc(vt_ni)
    if (present(vt_s)) out%vt_s = c_loc(vt_s)
    if (present(vt_g)) out%vt_g = c_loc(vt_g)
    if (present(flux_r)) out%flux_r = c_loc(flux_r)
    if (present(flux_i)) out%flux_i = c_loc(flux_i)
    if (present(flux_s)) out%flux_s = c_loc(flux_s)
    if (present(flux_g)) out%flux_g = c_loc(flux_g)
    if (present(flux_total)) out%flux_total = c_loc(flux_total)
    if (kind(t) == c_double) then
       rc = kidmp_fall_speeds_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqi, pni, pqs, pqg, pboost, pdz, 0_c_int64_t, dt8, out, pnstep)
    else
       rc = kidmp32_fall_speeds_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqi, pni, pqs, pqg, pboost, pdz, 0_c_int64_t, dt8, out, pnstep)
    end if
    call stop_on_error(rc, 'fall_speeds_batch')
  end subroutine fall_speeds_batch

  ! The size distributions of a state over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_spectra.h):
  ! per species (cloud water c, cloud ice i, rain r, snow s, graupel g) the spectrum n_x(nz, nb, ncol), particles per m3 of
  ! air in each diameter bin, and the parameters of the distribution (nz, ncol): slope and intercept lam_x, n0_x (nu_c for
  ! cloud water; smob and smoc for snow).  Every output is optional, in the array kind the arithmetic stores; at least one
  ! must be present.  A spectrum is put on the grid D_x(nb), dD_x(nb) (m, always REAL 8; 1 <= nb <= 256) when both are
  ! given, else on the scheme's own 100 bins, and its second extent must be that nb.  nc is read only by an aerosol-aware
  ! run; qi, ni, qs and qg may be left out in an iiwarm run or when no frozen output is asked for.  The inputs are not
  ! changed.  Default REAL 8 goes to kidmp_size_spectra_host, REAL 4 to kidmp32_...
  subroutine size_spectra_batch(ncol, nz, t, p, qv, qc, qr, nr, n_c, n_i, n_r, n_s, n_g, lam_c, n0_c, nu_c, lam_i, n0_i, &
       lam_r, n0_r, smob, smoc, lam_g, n0_g, nc, qi, ni, qs, qg, D_c, dD_c, D_i, dD_i, D_r, dD_r, D_s, dD_s, D_g, dD_g)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qc, qr, nr
    real, dimension(:,:,:), intent(inout), optional, target, contiguous :: n_c, n_i, n_r, n_s, n_g
    real, dimension(nz,ncol), intent(out), optional, target :: lam_c, n0_c, nu_c, lam_i, n0_i, lam_r, n0_r, smob, smoc, lam_g, n0_g
    real, dimension(nz,ncol), intent(in), optional, target :: nc, qi, ni, qs, qg
    real(c_double), dimension(:), intent(in), optional, target, contiguous :: D_c, dD_c, D_i, dD_i, D_r, dD_r, D_s, dD_s, D_g, dD_g
    type(kidmp_spectra_out) :: par
    type(kidmp_spectra_bins) :: bins
    type(kidmp_spectra_grids) :: grids
    type(c_ptr) :: pnc, pqi, pni, pqs, pqg, pn(5)
    integer(c_int) :: rc
    integer :: x
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: size spectra are not available with kidmp_ndevices > 1'
       stop 1
    end if
    pnc = c_null_ptr;  pqi = c_null_ptr;  pni = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr
    if (present(nc)) pnc = c_loc(nc)
    if (present(qi)) pqi = c_loc(qi)
    if (present(ni)) pni = c_loc(ni)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    do x = 1, 5
       grids%D(x) = c_null_ptr;  grids%dD(x) = c_null_ptr;  grids%nb(x) = 0_c_int32_t
    end do
    call species(1, n_c, D_c, dD_c)
    call species(2, n_i, D_i, dD_i)
    call species(3, n_r, D_r, dD_r)
    call species(4, n_s, D_s, dD_s)
    call species(5, n_g, D_g, dD_g)
    bins = kidmp_spectra_bins(pn(1), pn(2), pn(3), pn(4), pn(5))
    par = kidmp_spectra_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(lam_c)) par%lam_c = c_loc(lam_c)
    if (present(n0_c)) par%n0_c = c_loc(n0_c)
    if (present(nu_c)) par%nu_c = c_loc(nu_c)
    if (present(lam_i)) par%lam_i = c_loc(lam_i)
    if (present(n0_i)) par%n0_i = c_loc(n0_i)
    if (present(lam_r)) par%lam_r = c_loc(lam_r)
    if (present(n0_r)) par%n0_r = c_loc(n0_r)
    if (present(smob)) par%smob = c_loc(smob)
    if (present(smoc)) par%smoc = c_loc(smoc)
    if (present(lam_g)) par%lam_g = c_loc(lam_g)
    if (present(n0_g)) par%n0_g = c_loc(n0_g)
    if (kind(t) == c_double) then
       rc = kidmp_size_spectra_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), &
            pnc, pqi, pni, c_loc(qr), c_loc(nr), pqs, pqg, par, bins, grids)
    else
       rc = kidmp32_size_spectra_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), &
            pnc, pqi, pni, c_loc(qr), c_loc(nr), pqs, pqg, par, bins, grids)
    end if
    call stop_on_error(rc, 'size_spectra_batch')
  contains
    ! one species: the spectrum's address and, when the caller gives one, its grid; the extents are checked here, where
    ! they are known
    subroutine species(x, n, D, dD)
      integer, intent(in) :: x
      real, dimension(:,:,:), intent(inout), optional, target, contiguous :: n
      real(c_double), dimension(:), intent(in), optional, target, contiguous :: D, dD
      pn(x) = c_null_ptr
      if (.not. present(n)) return
      if (present(D) .neqv. present(dD)) call bad('a grid needs both D and dD')
      if (size(n, 1) /= nz .or. size(n, 3) /= ncol) call bad('a spectrum must be (nz, nb, ncol)')
      if (present(D)) then
         if (size(D) /= size(n, 2) .or. size(dD) /= size(n, 2)) call bad('D, dD and the spectrum differ in the number of bins')
         grids%D(x) = c_loc(D);  grids%dD(x) = c_loc(dD);  grids%nb(x) = int(size(D), c_int32_t)
      else if (size(n, 2) /= 100) then
         call bad('a spectrum on the scheme''s own grid has 100 bins')
      end if
      pn(x) = c_loc(n)
    end subroutine species
    subroutine bad(msg)
      character(*), intent(in) :: msg
      write(*,'(2a)') ' module_mp_thompson09n: size_spectra_batch: ', msg
      stop 1
    end subroutine bad
  end subroutine size_spectra_batch

  ! The radar moments of a state over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_doppler.h):
  ! reflectivity dbz (dBZ), mean Doppler velocity vd and spectrum width sw (m s-1, positive downward), and the per-species
  ! parts vz_r, vz_s, vz_g (m s-1) and dbz_r, dbz_s, dbz_g they are formed from.  Every output is optional, in the array
  ! kind the arithmetic stores; at least one must be present.  qs and qg left out mean zero; w is the vertical air velocity
  ! (positive upward), left out: still air.  A level without rain, snow and graupel has vd = sw = 0.  The inputs are not
  ! changed.  Default REAL 8 goes to kidmp_doppler_moments_host, REAL 4 to kidmp32_...
  subroutine doppler_moments_batch(ncol, nz, t, p, qv, qr, nr, dbz, vd, sw, vz_r, vz_s, vz_g, dbz_r, dbz_s, dbz_g, qs, qg, w)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: dbz, vd, sw, vz_r, vz_s, vz_g, dbz_r, dbz_s, dbz_g
    real, dimension(nz,ncol), intent(in), optional, target :: qs, qg, w
    type(kidmp_doppler_out) :: out
    type(c_ptr) :: pqs, pqg, pw
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: Doppler moments are not available with kidmp_ndevices > 1'
       stop 1
    end if
    pqs = c_null_ptr;  pqg = c_null_ptr;  pw = c_null_ptr
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(w)) pw = c_loc(w)
    out = kidmp_doppler_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr)
    if (present(dbz)) out%dbz = c_loc(dbz)
    if (present(vd)) out%vd = c_loc(vd)
    if (present(sw)) out%sw = c_loc(sw)
    if (present(vz_r)) out%vz_r = c_loc(vz_r)
    if (present(vz_s)) out%vz_s = c_loc(vz_s)
    if (present(vz_g)) out%vz_g = c_loc(vz_g)
    if (present(dbz_r)) out%dbz_r = c_loc(dbz_r)
    if (present(dbz_s)) out%dbz_s = c_loc(dbz_s)
    if (present(dbz_g)) out%dbz_g = c_loc(dbz_g)
    if (kind(t) == c_double) then
       rc = kidmp_doppler_moments_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pw, out)
    else
       rc = kidmp32_doppler_moments_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pw, out)
    end if
    call stop_on_error(rc, 'doppler_moments_batch')
  end subroutine doppler_moments_batch

  ! The lidar operator of include/kidmp_lidar.h over ncol columns of KiD's (nz, ncol) storage in one call: the extinction of
  ! the five species, of all particles and their backscatter, the molecular backscatter, the optical depth and the
  ! layer-mean attenuated backscatter seen from the ground (_up) and from space (_dn), and the scattering ratios.  Every
  ! output is optional, the profiles in the array kind the arithmetic stores; summary(s+1, i) is slot s of column i, always
  ! real(c_double); at least one must be present.  dz(nz) is KiD's one profile of layer depths.  nc may be left out unless
  ! is_aerosol_aware, qi, ni, qs and qg in an iiwarm run.  A member of the configuration left out keeps the library's
  ! convention (s_ratio = 18.8, 25, 18.8, 25, 25 for c, i, r, s, g; eta 0.7; c_mol 6.2446e-32; beta_detect 2e-5; trans_lost
  ! 2.5e-3).  The inputs are not changed.  Default REAL 8 goes to kidmp_lidar_profiles_host, REAL 4 to kidmp32_...
  subroutine lidar_profiles_batch(ncol, nz, t, p, qv, qc, qr, nr, dz, ext_c, ext_i, ext_r, ext_s, ext_g, ext, bsc, bsc_mol, &
       tau_up, tau_dn, att_up, att_dn, sr_up, sr_dn, summary, nc, qi, ni, qs, qg, s_ratio, eta, c_mol, beta_detect, trans_lost)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qc, qr, nr
    real, dimension(nz), intent(in), target :: dz
    real, dimension(nz,ncol), intent(out), optional, target :: ext_c, ext_i, ext_r, ext_s, ext_g, ext, bsc, bsc_mol, &
         tau_up, tau_dn, att_up, att_dn, sr_up, sr_dn
    real(c_double), dimension(8,ncol), intent(out), optional, target :: summary
    real, dimension(nz,ncol), intent(in), optional, target :: nc, qi, ni, qs, qg
    real(c_double), intent(in), optional :: s_ratio(5), eta, c_mol, beta_detect, trans_lost
    real(c_double), target :: cfg(9)                       ! kidmp_lidar_cfg: nine doubles
    type(kidmp_lidar_out) :: out
    type(c_ptr) :: pnc, pqi, pni, pqs, pqg, pcfg, psum
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: lidar profiles are not available with kidmp_ndevices > 1'
       stop 1
    end if
    pnc = c_null_ptr;  pqi = c_null_ptr;  pni = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr
    pcfg = c_null_ptr;  psum = c_null_ptr
    if (present(nc)) pnc = c_loc(nc)
    if (present(qi)) pqi = c_loc(qi)
    if (present(ni)) pni = c_loc(ni)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(summary)) psum = c_loc(summary)
    if (present(s_ratio) .or. present(eta) .or. present(c_mol) .or. present(beta_detect) .or. present(trans_lost)) then
       cfg = (/ 18.8_c_double, 25.0_c_double, 18.8_c_double, 25.0_c_double, 25.0_c_double, 0.7_c_double, 6.2446e-32_c_double, &
            2.0e-5_c_double, 2.5e-3_c_double /)
       if (present(s_ratio)) cfg(1:5) = s_ratio
       if (present(eta)) cfg(6) = eta
       if (present(c_mol)) cfg(7) = c_mol
       if (present(beta_detect)) cfg(8) = beta_detect
       if (present(trans_lost)) cfg(9) = trans_lost
       pcfg = c_loc(cfg)
    end if
    out = kidmp_lidar_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(ext_c)) out%ext_c = c_loc(ext_c)
    if (present(ext_i)) out%ext_i = c_loc(ext_i)
    if (present(ext_r)) out%ext_r = c_loc(ext_r)
    if (present(ext_s)) out%ext_s = c_loc(ext_s)
    if (present(ext_g)) out%ext_g = c_loc(ext_g)
    if (present(ext)) out%ext = c_loc(ext)
    if (present(bsc)) out%bsc = c_loc(bsc)
    if (present(bsc_mol)) out%bsc_mol = c_loc(bsc_mol)
    if (present(tau_up)) out%tau_up = c_loc(tau_up)
    if (present(tau_dn)) out%tau_dn = c_loc(tau_dn)
    if (present(att_up)) out%att_up = c_loc(att_up)
    if (present(att_dn)) out%att_dn = c_loc(att_dn)
    if (present(sr_up)) out%sr_up = c_loc(sr_up)
    if (present(sr_dn)) out%sr_dn = c_loc(sr_dn)
    if (kind(t) == c_double) then
       rc = kidmp_lidar_profiles_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), &
            pnc, pqi, pni, c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dz), 0_c_int64_t, pcfg, out, psum)
    else
       rc = kidmp32_lidar_profiles_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qc), &
            pnc, pqi, pni, c_loc(qr), c_loc(nr), pqs, pqg, c_loc(dz), 0_c_int64_t, pcfg, out, psum)
    end if
    call stop_on_error(rc, 'lidar_profiles_batch')
  end subroutine lidar_profiles_batch

  ! The Doppler spectrum of a state over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_dspectrum.h):
  ! the reflectivity (m6 m-3 per bin) of rain, snow and graupel together (total) and apart, as spectra (nz, nv, ncol) on the
  ! uniform velocity grid v0 + j*dv, j = 0 .. nv-1 (m s-1, positive downward, always REAL 8; 1 <= nv <= 256), and what total
  ! holds outside the grid, below and above (nz, ncol).  Every output is optional, in the array kind the arithmetic stores;
  ! at least one must be present, and the second extent of a spectrum must be nv.  qs and qg left out mean zero; w is the
  ! vertical air velocity (positive upward), left out: still air.  A species is put on the diameter grid D_x(nb), dD_x(nb)
  ! (m, always REAL 8; 1 <= nb <= 256) when both are given, else on the scheme's own 100 bins.  The inputs are not
  ! changed.  Default REAL 8 goes to kidmp_doppler_spectrum_host, REAL 4 to kidmp32_...
  subroutine doppler_spectrum_batch(ncol, nz, t, p, qv, qr, nr, v0, dv, nv, total, rain, snow, graupel, below, above, qs, qg, w, &
       D_r, dD_r, D_s, dD_s, D_g, dD_g)
    integer, intent(in) :: ncol, nz, nv
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real(c_double), intent(in) :: v0, dv
    real, dimension(:,:,:), intent(inout), optional, target, contiguous :: total, rain, snow, graupel
    real, dimension(nz,ncol), intent(out), optional, target :: below, above
    real, dimension(nz,ncol), intent(in), optional, target :: qs, qg, w
    real(c_double), dimension(:), intent(in), optional, target, contiguous :: D_r, dD_r, D_s, dD_s, D_g, dD_g
    type(kidmp_dspectrum_out) :: out
    type(kidmp_dspectrum_grids) :: grids
    type(c_ptr) :: pqs, pqg, pw
    integer(c_int) :: rc
    integer :: x
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: Doppler spectra are not available with kidmp_ndevices > 1'
       stop 1
    end if
    pqs = c_null_ptr;  pqg = c_null_ptr;  pw = c_null_ptr
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(w)) pw = c_loc(w)
    do x = 1, 3
       grids%D(x) = c_null_ptr;  grids%dD(x) = c_null_ptr;  grids%nb(x) = 0_c_int32_t
    end do
    call grid(1, D_r, dD_r)
    call grid(2, D_s, dD_s)
    call grid(3, D_g, dD_g)
    out = kidmp_dspectrum_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    call spectrum(out%total, total)
    call spectrum(out%rain, rain)
    call spectrum(out%snow, snow)
    call spectrum(out%graupel, graupel)
    if (present(below)) out%below = c_loc(below)
    if (present(above)) out%above = c_loc(above)
    if (kind(t) == c_double) then
       rc = kidmp_doppler_spectrum_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pw, v0, dv, int(nv, c_int32_t), grids, out)
    else
       rc = kidmp32_doppler_spectrum_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pw, v0, dv, int(nv, c_int32_t), grids, out)
    end if
    call stop_on_error(rc, 'doppler_spectrum_batch')
  contains
    ! one spectrum's address; its extents are checked here, where they are known
    subroutine spectrum(ptr, s)
      type(c_ptr), intent(inout) :: ptr
      real, dimension(:,:,:), intent(inout), optional, target, contiguous :: s
      if (.not. present(s)) return
      if (size(s, 1) /= nz .or. size(s, 2) /= nv .or. size(s, 3) /= ncol) call bad('a spectrum must be (nz, nv, ncol)')
      ptr = c_loc(s)
    end subroutine spectrum
    subroutine grid(x, D, dD)
      integer, intent(in) :: x
      real(c_double), dimension(:), intent(in), optional, target, contiguous :: D, dD
      if (present(D) .neqv. present(dD)) call bad('a grid needs both D and dD')
      if (.not. present(D)) return
      if (size(D) /= size(dD)) call bad('D and dD differ in the number of bins')
      grids%D(x) = c_loc(D);  grids%dD(x) = c_loc(dD);  grids%nb(x) = int(size(D), c_int32_t)
    end subroutine grid
    subroutine bad(msg)
      character(*), intent(in) :: msg
      write(*,'(2a)') ' module_mp_thompson09n: doppler_spectrum_batch: ', msg
      stop 1
    end subroutine bad
  end subroutine doppler_spectrum_batch

  ! calc_refl10cm with melting snow and graupel below the melting level, over ncol columns of KiD's (nz, ncol) storage in
  ! one call (include/kidmp_brightband.h): dbz and the per-species dbz_s, dbz_g (dBZ), the linear enhancements enh_s, enh_g
  ! (exactly 1.0 where the species is dry), the melt fractions fmelt_s, fmelt_g, all (nz, ncol) in the array kind the
  ! arithmetic stores, and the melting level k0(ncol) as the library counts it: 0-based, k0 + 1 is the Fortran level, -1 =
  ! none.  Every output is optional; at least one must be present.  qs and qg left out mean zero.  topology: 0 = water is
  ! the matrix (the default), 1 = the ice-air core is; the rest of the configuration keeps the library's defaults.  A
  ! species is put on the diameter grid D_x(nb), dD_x(nb) (m, always REAL 8; 1 <= nb <= 256) when both are given, else on
  ! the scheme's own 100 bins.  The inputs are not changed.  Default REAL 8 goes to kidmp_bright_band_host, REAL 4 to kidmp32_...
  subroutine bright_band_batch(ncol, nz, t, p, qv, qr, nr, dbz, dbz_s, dbz_g, enh_s, enh_g, fmelt_s, fmelt_g, k0, qs, qg, &
       topology, D_s, dD_s, D_g, dD_g)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: dbz, dbz_s, dbz_g, enh_s, enh_g, fmelt_s, fmelt_g
    integer(c_int32_t), dimension(ncol), intent(out), optional, target :: k0
    real, dimension(nz,ncol), intent(in), optional, target :: qs, qg
    integer, intent(in), optional :: topology
    real(c_double), dimension(:), intent(in), optional, target, contiguous :: D_s, dD_s, D_g, dD_g
    type(kidmp_brightband_out) :: out
    type(kidmp_brightband_grids) :: grids
    type(kidmp_brightband_cfg), target :: cfg
    type(c_ptr) :: pqs, pqg, pcfg
    integer(c_int) :: rc
    integer :: x
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the bright band is not available with kidmp_ndevices > 1'
       stop 1
    end if
    pqs = c_null_ptr;  pqg = c_null_ptr;  pcfg = c_null_ptr
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(topology)) then
       call kidmp_brightband_defaults(cfg)
       cfg%topology = int(topology, c_int32_t)
       pcfg = c_loc(cfg)
    end if
    do x = 1, 2
       grids%D(x) = c_null_ptr;  grids%dD(x) = c_null_ptr;  grids%nb(x) = 0_c_int32_t
    end do
    call grid(1, D_s, dD_s)
    call grid(2, D_g, dD_g)
    out = kidmp_brightband_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz)) out%dbz = c_loc(dbz)
    if (present(dbz_s)) out%dbz_s = c_loc(dbz_s)
    if (present(dbz_g)) out%dbz_g = c_loc(dbz_g)
    if (present(enh_s)) out%enh_s = c_loc(enh_s)
    if (present(enh_g)) out%enh_g = c_loc(enh_g)
    if (present(fmelt_s)) out%fmelt_s = c_loc(fmelt_s)
    if (present(fmelt_g)) out%fmelt_g = c_loc(fmelt_g)
    if (present(k0)) out%k0 = c_loc(k0)
    if (kind(t) == c_double) then
       rc = kidmp_bright_band_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pcfg, grids, out)
    else
       rc = kidmp32_bright_band_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), c_loc(qr), &
            c_loc(nr), pqs, pqg, pcfg, grids, out)
    end if
    call stop_on_error(rc, 'bright_band_batch')
  contains
    subroutine grid(x, D, dD)
      integer, intent(in) :: x
      real(c_double), dimension(:), intent(in), optional, target, contiguous :: D, dD
      if (present(D) .neqv. present(dD)) call bad('a grid needs both D and dD')
      if (.not. present(D)) return
      if (size(D) /= size(dD)) call bad('D and dD differ in the number of bins')
      grids%D(x) = c_loc(D);  grids%dD(x) = c_loc(dD);  grids%nb(x) = int(size(D), c_int32_t)
    end subroutine grid
    subroutine bad(msg)
      character(*), intent(in) :: msg
      write(*,'(2a)') ' module_mp_thompson09n: bright_band_batch: ', msg
      stop 1
    end subroutine bad
  end subroutine bright_band_batch

  ! The cloud radar over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_mie.h): Mie reflectivity, its
  ! per-species parts and their ratios mie_x to the Rayleigh reflectivity, the one-way extinction ext (1/m), the two-way
  ! path-integrated attenuation seen from the ground (pia_up) and from space (pia_down) with the attenuated dbz_up and
  ! dbz_down, the mean Doppler velocity vd, all (nz, ncol) in the array kind the arithmetic stores, and pia_total(ncol).
  ! Every output is optional; at least one must be present.  The configuration: wavelength (m) and the complex relative
  ! permittivities of water and ice at that wavelength are the caller's; rho_w, rho_i and kw2 keep the library's defaults
  ! when left out.  The table of Mie rows on the scheme's own bins is built for the call and freed after it: a caller of many
  ! batches at one wavelength pays some 300 spheres per call.  qc, qs, qg, w (nz, ncol) and k_gas(nz) left out mean zero;
  ! dz(nz) is needed for the path outputs.  The inputs are not changed.  Default REAL 8 goes to kidmp_mie_radar_host, REAL
  ! 4 to kidmp32_...
  subroutine mie_radar_batch(ncol, nz, wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, t, p, qv, qr, nr, dbz, dbz_up, &
       dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, mie_g, ext, pia_up, pia_down, vd, pia_total, qc, qs, qg, dz, w, k_gas, &
       rho_w, rho_i, kw2)
    integer, intent(in) :: ncol, nz
    real(c_double), intent(in) :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: dbz, dbz_up, dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, mie_g, &
         ext, pia_up, pia_down, vd
    real, dimension(ncol), intent(out), optional, target :: pia_total
    real, dimension(nz,ncol), intent(in), optional, target :: qc, qs, qg, w
    real, dimension(nz), intent(in), optional, target :: dz, k_gas
    real(c_double), intent(in), optional :: rho_w, rho_i, kw2
    type(kidmp_mie_out) :: out
    type(kidmp_mie_cfg) :: cfg
    type(c_ptr) :: table, pqc, pqs, pqg, pdz, pw, pkg
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the cloud radar is not available with kidmp_ndevices > 1'
       stop 1
    end if
    call kidmp_mie_defaults(cfg)
    cfg%wavelength = wavelength
    cfg%eps_w_re = eps_w_re;  cfg%eps_w_im = eps_w_im;  cfg%eps_i_re = eps_i_re;  cfg%eps_i_im = eps_i_im
    if (present(rho_w)) cfg%rho_w = rho_w
    if (present(rho_i)) cfg%rho_i = rho_i
    if (present(kw2)) cfg%kw2 = kw2
    pqc = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pdz = c_null_ptr;  pw = c_null_ptr;  pkg = c_null_ptr
    if (present(qc)) pqc = c_loc(qc)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(dz)) pdz = c_loc(dz)
    if (present(w)) pw = c_loc(w)
    if (present(k_gas)) pkg = c_loc(k_gas)
    out = kidmp_mie_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz)) out%dbz = c_loc(dbz)
    if (present(dbz_up)) out%dbz_up = c_loc(dbz_up)
    if (present(dbz_down)) out%dbz_down = c_loc(dbz_down)
    if (present(dbz_r)) out%dbz_r = c_loc(dbz_r)
    if (present(dbz_s)) out%dbz_s = c_loc(dbz_s)
    if (present(dbz_g)) out%dbz_g = c_loc(dbz_g)
    if (present(mie_r)) out%mie_r = c_loc(mie_r)
    if (present(mie_s)) out%mie_s = c_loc(mie_s)
    if (present(mie_g)) out%mie_g = c_loc(mie_g)
    if (present(ext)) out%ext = c_loc(ext)
    if (present(pia_up)) out%pia_up = c_loc(pia_up)
    if (present(pia_down)) out%pia_down = c_loc(pia_down)
    if (present(vd)) out%vd = c_loc(vd)
    if (present(pia_total)) out%pia_total = c_loc(pia_total)
    rc = kidmp_mie_table_create(ctx, cfg, c_null_ptr, table)
    call stop_on_error(rc, 'mie_radar_batch (table)')
    if (kind(t) == c_double) then
       rc = kidmp_mie_radar_host(ctx, table, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), pqc, &
            c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pw, pkg, 0_c_int64_t, out)
    else
       rc = kidmp32_mie_radar_host(ctx, table, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), pqc, &
            c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pw, pkg, 0_c_int64_t, out)
    end if
    call kidmp_mie_table_destroy(table)
    call stop_on_error(rc, 'mie_radar_batch')
  end subroutine mie_radar_batch

  ! The microwave radiometer over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_radiometer.h): the
  ! absorption and back-hemisphere scattering coefficients k_abs, k_bsc (1/m), the two-stream layer's refl and trans, the
  ! brightness temperatures going up through the upper face (tb_up) and coming down through the lower face (tb_down) of
  ! every level, all (nz, ncol) in the array kind the arithmetic stores, and per column tb_toa (what a satellite sees),
  ! tb_ground (what a ground radiometer sees) and tau_abs.  Every output is optional; at least one must be present.  The
  ! configuration is mie_radar_batch's (kw2 is not read); mu, emissivity and t_cosmic keep the library's 1, 1 and 2.725 K
  ! when left out.  The table on the scheme's own bins is built for the call and freed after it.  qc, qs, qg (nz, ncol) and
  ! k_gas(nz) left out mean zero; t_sfc(ncol) left out means the column's t at the lowest level; dz(nz) is needed for
  ! everything but k_abs and k_bsc.  The inputs are not changed.  Default REAL 8 goes to kidmp_radiometer_host, REAL 4 to
  ! kidmp32_...
  subroutine radiometer_batch(ncol, nz, wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, t, p, qv, qr, nr, k_abs, k_bsc, &
       refl, trans, tb_up, tb_down, tb_toa, tb_ground, tau_abs, qc, qs, qg, dz, k_gas, t_sfc, rho_w, rho_i, mu, emissivity, &
       t_cosmic)
    integer, intent(in) :: ncol, nz
    real(c_double), intent(in) :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: k_abs, k_bsc, refl, trans, tb_up, tb_down
    real, dimension(ncol), intent(out), optional, target :: tb_toa, tb_ground, tau_abs
    real, dimension(nz,ncol), intent(in), optional, target :: qc, qs, qg
    real, dimension(nz), intent(in), optional, target :: dz, k_gas
    real, dimension(ncol), intent(in), optional, target :: t_sfc
    real(c_double), intent(in), optional :: rho_w, rho_i, mu, emissivity, t_cosmic
    type(kidmp_radiometer_out) :: out
    type(kidmp_radiometer_cfg) :: rcfg
    type(kidmp_mie_cfg) :: cfg
    type(c_ptr) :: table, pqc, pqs, pqg, pdz, pkg, pts
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the radiometer is not available with kidmp_ndevices > 1'
       stop 1
    end if
    call kidmp_mie_defaults(cfg)
    cfg%wavelength = wavelength
    cfg%eps_w_re = eps_w_re;  cfg%eps_w_im = eps_w_im;  cfg%eps_i_re = eps_i_re;  cfg%eps_i_im = eps_i_im
    if (present(rho_w)) cfg%rho_w = rho_w
    if (present(rho_i)) cfg%rho_i = rho_i
    call kidmp_radiometer_defaults(rcfg)
    if (present(mu)) rcfg%mu = mu
    if (present(emissivity)) rcfg%emissivity = emissivity
    if (present(t_cosmic)) rcfg%t_cosmic = t_cosmic
    pqc = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pdz = c_null_ptr;  pkg = c_null_ptr;  pts = c_null_ptr
    if (present(qc)) pqc = c_loc(qc)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(dz)) pdz = c_loc(dz)
    if (present(k_gas)) pkg = c_loc(k_gas)
    if (present(t_sfc)) pts = c_loc(t_sfc)
    out = kidmp_radiometer_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr)
    if (present(k_abs)) out%k_abs = c_loc(k_abs)
    if (present(k_bsc)) out%k_bsc = c_loc(k_bsc)
    if (present(refl)) out%refl = c_loc(refl)
    if (present(trans)) out%trans = c_loc(trans)
    if (present(tb_up)) out%tb_up = c_loc(tb_up)
    if (present(tb_down)) out%tb_down = c_loc(tb_down)
    if (present(tb_toa)) out%tb_toa = c_loc(tb_toa)
    if (present(tb_ground)) out%tb_ground = c_loc(tb_ground)
    if (present(tau_abs)) out%tau_abs = c_loc(tau_abs)
    rc = kidmp_radiometer_table_create(ctx, cfg, c_null_ptr, table)
    call stop_on_error(rc, 'radiometer_batch (table)')
    if (kind(t) == c_double) then
       rc = kidmp_radiometer_host(ctx, table, rcfg, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), pqc, &
            c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pkg, 0_c_int64_t, pts, out)
    else
       rc = kidmp32_radiometer_host(ctx, table, rcfg, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), pqc, &
            c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pkg, 0_c_int64_t, pts, out)
    end if
    call kidmp_radiometer_table_destroy(table)
    call stop_on_error(rc, 'radiometer_batch')
  end subroutine radiometer_batch

  ! radiometer_batch at nch channels in one launch per chunk of columns (include/kidmp_multichannel.h): the configuration is
  ! an array of nch wavelengths and permittivities, the outputs are (nz, ncol, nch) and (ncol, nch), and channel c holds the
  ! bits radiometer_batch gives with the c-th configuration.  k_gas is (nz) for all channels or, as k_gas_ch(nz, nch), one
  ! profile per channel; mu, emissivity and t_cosmic are one value per channel and keep the library's defaults when left
  ! out; rho_w and rho_i are shared.  The nch tables are built for the call and freed after it.  1 <= nch <= 16.
  subroutine radiometer_multi_batch(nch, ncol, nz, wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, t, p, qv, qr, nr, k_abs, &
       k_bsc, refl, trans, tb_up, tb_down, tb_toa, tb_ground, tau_abs, qc, qs, qg, dz, k_gas, k_gas_ch, t_sfc, rho_w, rho_i, mu, &
       emissivity, t_cosmic)
    integer, intent(in) :: nch, ncol, nz
    real(c_double), dimension(nch), intent(in) :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol,nch), intent(out), optional, target :: k_abs, k_bsc, refl, trans, tb_up, tb_down
    real, dimension(ncol,nch), intent(out), optional, target :: tb_toa, tb_ground, tau_abs
    real, dimension(nz,ncol), intent(in), optional, target :: qc, qs, qg
    real, dimension(nz), intent(in), optional, target :: dz, k_gas
    real, dimension(nz,nch), intent(in), optional, target :: k_gas_ch
    real, dimension(ncol), intent(in), optional, target :: t_sfc
    real(c_double), intent(in), optional :: rho_w, rho_i
    real(c_double), dimension(nch), intent(in), optional :: mu, emissivity, t_cosmic
    type(kidmp_radiometer_out) :: out
    type(kidmp_radiometer_cfg) :: rcfg(nch)
    type(kidmp_mie_cfg) :: cfg
    type(c_ptr) :: tables(nch), pqc, pqs, pqg, pdz, pkg, pts
    integer(c_int64_t) :: kg_ch
    integer(c_int) :: rc
    integer :: c, made
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the radiometer is not available with kidmp_ndevices > 1'
       stop 1
    end if
    if (nch < 1 .or. nch > 16 .or. (present(k_gas) .and. present(k_gas_ch))) then
       write(*,'(a)') ' module_mp_thompson09n: radiometer_multi_batch: nch outside [1, 16], or both k_gas and k_gas_ch'
       stop 1
    end if
    do c = 1, nch
       call kidmp_radiometer_defaults(rcfg(c))
       if (present(mu)) rcfg(c)%mu = mu(c)
       if (present(emissivity)) rcfg(c)%emissivity = emissivity(c)
       if (present(t_cosmic)) rcfg(c)%t_cosmic = t_cosmic(c)
    end do
    pqc = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pdz = c_null_ptr;  pkg = c_null_ptr;  pts = c_null_ptr
    kg_ch = 0
    if (present(qc)) pqc = c_loc(qc)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(dz)) pdz = c_loc(dz)
    if (present(k_gas)) pkg = c_loc(k_gas)
    if (present(k_gas_ch)) then
       pkg = c_loc(k_gas_ch)
       kg_ch = nz
    end if
    if (present(t_sfc)) pts = c_loc(t_sfc)
    out = kidmp_radiometer_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr)
    if (present(k_abs)) out%k_abs = c_loc(k_abs)
    if (present(k_bsc)) out%k_bsc = c_loc(k_bsc)
    if (present(refl)) out%refl = c_loc(refl)
    if (present(trans)) out%trans = c_loc(trans)
    if (present(tb_up)) out%tb_up = c_loc(tb_up)
    if (present(tb_down)) out%tb_down = c_loc(tb_down)
    if (present(tb_toa)) out%tb_toa = c_loc(tb_toa)
    if (present(tb_ground)) out%tb_ground = c_loc(tb_ground)
    if (present(tau_abs)) out%tau_abs = c_loc(tau_abs)
    rc = 0
    made = 0
    do c = 1, nch
       call kidmp_mie_defaults(cfg)
       cfg%wavelength = wavelength(c)
       cfg%eps_w_re = eps_w_re(c);  cfg%eps_w_im = eps_w_im(c);  cfg%eps_i_re = eps_i_re(c);  cfg%eps_i_im = eps_i_im(c)
       if (present(rho_w)) cfg%rho_w = rho_w
       if (present(rho_i)) cfg%rho_i = rho_i
       rc = kidmp_radiometer_table_create(ctx, cfg, c_null_ptr, tables(c))
       if (rc < 0) exit
       made = c
    end do
    if (rc >= 0) then
       if (kind(t) == c_double) then
          rc = kidmp_radiometer_multi_host(ctx, tables, int(nch, c_int32_t), rcfg, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), &
               c_loc(p), c_loc(qv), pqc, c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pkg, 0_c_int64_t, kg_ch, pts, out)
       else
          rc = kidmp32_radiometer_multi_host(ctx, tables, int(nch, c_int32_t), rcfg, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), &
               c_loc(p), c_loc(qv), pqc, c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pkg, 0_c_int64_t, kg_ch, pts, out)
       end if
    end if
    do c = 1, made
       call kidmp_radiometer_table_destroy(tables(c))
    end do
    call stop_on_error(rc, 'radiometer_multi_batch')
  end subroutine radiometer_multi_batch

  ! mie_radar_batch at nch channels in one launch per chunk of columns (include/kidmp_multichannel.h), shaped as
  ! radiometer_multi_batch: profiles (nz, ncol, nch), pia_total (ncol, nch), kw2 one value per channel.  A dual-wavelength
  ! ratio is dbz(:,:,i) - dbz(:,:,j) on the result.
  subroutine mie_radar_multi_batch(nch, ncol, nz, wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, t, p, qv, qr, nr, dbz, &
       dbz_up, dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, mie_g, ext, pia_up, pia_down, vd, pia_total, qc, qs, qg, dz, w, k_gas, &
       k_gas_ch, rho_w, rho_i, kw2)
    integer, intent(in) :: nch, ncol, nz
    real(c_double), dimension(nch), intent(in) :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol,nch), intent(out), optional, target :: dbz, dbz_up, dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, &
         mie_g, ext, pia_up, pia_down, vd
    real, dimension(ncol,nch), intent(out), optional, target :: pia_total
    real, dimension(nz,ncol), intent(in), optional, target :: qc, qs, qg, w
    real, dimension(nz), intent(in), optional, target :: dz, k_gas
    real, dimension(nz,nch), intent(in), optional, target :: k_gas_ch
    real(c_double), intent(in), optional :: rho_w, rho_i
    real(c_double), dimension(nch), intent(in), optional :: kw2
    type(kidmp_mie_out) :: out
    type(kidmp_mie_cfg) :: cfg
    type(c_ptr) :: tables(nch), pqc, pqs, pqg, pdz, pw, pkg
    integer(c_int64_t) :: kg_ch
    integer(c_int) :: rc
    integer :: c, made
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the cloud radar is not available with kidmp_ndevices > 1'
       stop 1
    end if
    if (nch < 1 .or. nch > 16 .or. (present(k_gas) .and. present(k_gas_ch))) then
       write(*,'(a)') ' module_mp_thompson09n: mie_radar_multi_batch: nch outside [1, 16], or both k_gas and k_gas_ch'
       stop 1
    end if
    pqc = c_null_ptr;  pqs = c_null_ptr;  pqg = c_null_ptr;  pdz = c_null_ptr;  pw = c_null_ptr;  pkg = c_null_ptr
    kg_ch = 0
    if (present(qc)) pqc = c_loc(qc)
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    if (present(dz)) pdz = c_loc(dz)
    if (present(w)) pw = c_loc(w)
    if (present(k_gas)) pkg = c_loc(k_gas)
    if (present(k_gas_ch)) then
       pkg = c_loc(k_gas_ch)
       kg_ch = nz
    end if
    out = kidmp_mie_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz)) out%dbz = c_loc(dbz)
    if (present(dbz_up)) out%dbz_up = c_loc(dbz_up)
    if (present(dbz_down)) out%dbz_down = c_loc(dbz_down)
    if (present(dbz_r)) out%dbz_r = c_loc(dbz_r)
    if (present(dbz_s)) out%dbz_s = c_loc(dbz_s)
    if (present(dbz_g)) out%dbz_g = c_loc(dbz_g)
    if (present(mie_r)) out%mie_r = c_loc(mie_r)
    if (present(mie_s)) out%mie_s = c_loc(mie_s)
    if (present(mie_g)) out%mie_g = c_loc(mie_g)
    if (present(ext)) out%ext = c_loc(ext)
    if (present(pia_up)) out%pia_up = c_loc(pia_up)
    if (present(pia_down)) out%pia_down = c_loc(pia_down)
    if (present(vd)) out%vd = c_loc(vd)
    if (present(pia_total)) out%pia_total = c_loc(pia_total)
    rc = 0
    made = 0
    do c = 1, nch
       call kidmp_mie_defaults(cfg)
       cfg%wavelength = wavelength(c)
       cfg%eps_w_re = eps_w_re(c);  cfg%eps_w_im = eps_w_im(c);  cfg%eps_i_re = eps_i_re(c);  cfg%eps_i_im = eps_i_im(c)
       if (present(rho_w)) cfg%rho_w = rho_w
       if (present(rho_i)) cfg%rho_i = rho_i
       if (present(kw2)) cfg%kw2 = kw2(c)
       rc = kidmp_mie_table_create(ctx, cfg, c_null_ptr, tables(c))
       if (rc < 0) exit
       made = c
    end do
    if (rc >= 0) then
       if (kind(t) == c_double) then
          rc = kidmp_mie_radar_multi_host(ctx, tables, int(nch, c_int32_t), int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), &
               c_loc(qv), pqc, c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pw, pkg, 0_c_int64_t, kg_ch, out)
       else
          rc = kidmp32_mie_radar_multi_host(ctx, tables, int(nch, c_int32_t), int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), &
               c_loc(qv), pqc, c_loc(qr), c_loc(nr), pqs, pqg, pdz, 0_c_int64_t, pw, pkg, 0_c_int64_t, kg_ch, out)
       end if
    end if
    do c = 1, made
       call kidmp_mie_table_destroy(tables(c))
    end do
    call stop_on_error(rc, 'mie_radar_multi_batch')
  end subroutine mie_radar_multi_batch

  ! The polarimetric radar over ncol columns of KiD's (nz, ncol) storage in one call (include/kidmp_polarimetric.h): the
  ! reflectivity at horizontal polarisation dbz_h (dBZ), the differential reflectivity zdr (dB), the specific differential
  ! phase kdp (degrees per km) and the co-polar correlation rhohv of oblate spheroids in the Rayleigh-Gans approximation,
  ! with the parts of rain, snow and graupel, all (nz, ncol) in the array kind the arithmetic stores.  Every output is
  ! optional; at least one must be present.  The wavelength, the permittivities and the densities keep kidmp_mie_defaults'
  ! 10 cm when left out; the axis ratios (axis_r(5) the coefficients of rain's law in mm, axis_r_min, axis_s, axis_g), the
  ! canting widths sigma(3) in radians and force_quadrature keep kidmp_pol_defaults' illustrative values.  The table on the
  ! scheme's own bins is built for the call and freed after it.  qs, qg (nz, ncol) left out mean zero.  The inputs are not
  ! changed.  Default REAL 8 goes to kidmp_polarimetric_host, REAL 4 to kidmp32_...
  subroutine polarimetric_batch(ncol, nz, t, p, qv, qr, nr, dbz_h, zdr, kdp, rhohv, dbz_h_r, dbz_h_s, dbz_h_g, zdr_r, zdr_s, &
       zdr_g, kdp_r, kdp_s, kdp_g, qs, qg, wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, rho_w, rho_i, axis_r, &
       axis_r_min, axis_s, axis_g, sigma, force_quadrature)
    integer, intent(in) :: ncol, nz
    real, dimension(nz,ncol), intent(in), target :: t, p, qv, qr, nr
    real, dimension(nz,ncol), intent(out), optional, target :: dbz_h, zdr, kdp, rhohv, dbz_h_r, dbz_h_s, dbz_h_g, zdr_r, zdr_s, &
         zdr_g, kdp_r, kdp_s, kdp_g
    real, dimension(nz,ncol), intent(in), optional, target :: qs, qg
    real(c_double), intent(in), optional :: wavelength, eps_w_re, eps_w_im, eps_i_re, eps_i_im, rho_w, rho_i
    real(c_double), intent(in), optional :: axis_r(5), axis_r_min, axis_s, axis_g, sigma(3)
    logical, intent(in), optional :: force_quadrature
    type(kidmp_pol_out) :: out
    type(kidmp_mie_cfg) :: cfg
    type(kidmp_pol_cfg) :: pcfg
    type(c_ptr) :: table, pqs, pqg
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: the polarimetric radar is not available with kidmp_ndevices > 1'
       stop 1
    end if
    call kidmp_mie_defaults(cfg)
    if (present(wavelength)) cfg%wavelength = wavelength
    if (present(eps_w_re)) cfg%eps_w_re = eps_w_re
    if (present(eps_w_im)) cfg%eps_w_im = eps_w_im
    if (present(eps_i_re)) cfg%eps_i_re = eps_i_re
    if (present(eps_i_im)) cfg%eps_i_im = eps_i_im
    if (present(rho_w)) cfg%rho_w = rho_w
    if (present(rho_i)) cfg%rho_i = rho_i
    call kidmp_pol_defaults(pcfg)
    if (present(axis_r)) pcfg%axis_r = axis_r
    if (present(axis_r_min)) pcfg%axis_r_min = axis_r_min
    if (present(axis_s)) pcfg%axis_s = axis_s
    if (present(axis_g)) pcfg%axis_g = axis_g
    if (present(sigma)) pcfg%sigma = sigma
    if (present(force_quadrature)) pcfg%force_quadrature = merge(1_c_int32_t, 0_c_int32_t, force_quadrature)
    pqs = c_null_ptr;  pqg = c_null_ptr
    if (present(qs)) pqs = c_loc(qs)
    if (present(qg)) pqg = c_loc(qg)
    out = kidmp_pol_out(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
         c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz_h)) out%dbz_h = c_loc(dbz_h)
    if (present(zdr)) out%zdr = c_loc(zdr)
    if (present(kdp)) out%kdp = c_loc(kdp)
    if (present(rhohv)) out%rhohv = c_loc(rhohv)
    if (present(dbz_h_r)) out%dbz_h_r = c_loc(dbz_h_r)
    if (present(dbz_h_s)) out%dbz_h_s = c_loc(dbz_h_s)
    if (present(dbz_h_g)) out%dbz_h_g = c_loc(dbz_h_g)
    if (present(zdr_r)) out%zdr_r = c_loc(zdr_r)
    if (present(zdr_s)) out%zdr_s = c_loc(zdr_s)
    if (present(zdr_g)) out%zdr_g = c_loc(zdr_g)
    if (present(kdp_r)) out%kdp_r = c_loc(kdp_r)
    if (present(kdp_s)) out%kdp_s = c_loc(kdp_s)
    if (present(kdp_g)) out%kdp_g = c_loc(kdp_g)
    rc = kidmp_pol_table_create(ctx, cfg, pcfg, c_null_ptr, table)
    call stop_on_error(rc, 'polarimetric_batch (table)')
    if (kind(t) == c_double) then
       rc = kidmp_polarimetric_host(ctx, table, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qr), c_loc(nr), pqs, pqg, out)
    else
       rc = kidmp32_polarimetric_host(ctx, table, int(ncol, c_int64_t), int(nz, c_int32_t), c_loc(t), c_loc(p), c_loc(qv), &
            c_loc(qr), c_loc(nr), pqs, pqg, out)
    end if
    call kidmp_pol_table_destroy(table)
    call stop_on_error(rc, 'polarimetric_batch')
  end subroutine polarimetric_batch

  ! A droplet number per column (kidmp_set_column_nc): column i of every following batched call uses Nt_c =
  ! set_nc_col(i)*1.e6 (M:381) in place of the namelist's set_Nc -- an Nd ensemble, or an aerosol gradient along x, in
  ! one launch.  cm**-3 like set_Nc; the values are copied.  An absent or zero-size argument unbinds.  While bound, a
  ! batched call must have exactly size(set_nc_col) columns; not with is_aerosol_aware, not on several devices.
  subroutine mp_thompson_set_column_nc(set_nc_col)
    real, intent(in), optional :: set_nc_col(:)
    real(c_double), allocatable, target :: v(:)
    integer(c_int) :: rc
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: mp_thompson_set_column_nc is not available with kidmp_ndevices > 1'
       stop 1
    end if
    if (.not. present(set_nc_col)) then
       rc = kidmp_set_column_nc(ctx, 0_c_int64_t, c_null_ptr)
    else if (size(set_nc_col) == 0) then
       rc = kidmp_set_column_nc(ctx, 0_c_int64_t, c_null_ptr)
    else
       allocate(v(size(set_nc_col)))
       v = real(set_nc_col, c_double)
       rc = kidmp_set_column_nc(ctx, int(size(v), c_int64_t), c_loc(v))
    end if
    call stop_on_error(rc, 'mp_thompson_set_column_nc')
  end subroutine mp_thompson_set_column_nc

  ! The page-locked staging arrays themselves, for a caller whose default REAL is the storage type of kidmp_arith
  ! (8-byte REAL with 'p64', 4-byte REAL with 'p32n' / 'f32'): st(nz,ncol,12) in the argument order of mp_thompson
  ! (qv qc qi qr qs qg ni nr nc nwfa nifa t), fo(nz,ncol,3) = p, w, dz, pp(4,ncol).  Filled in place and passed to
  ! mp_thompson_batch -- ALL of them, slot by slot -- they are not copied again, in or out.  ok = .false. (and null
  ! pointers) when the kinds differ: the caller then brings its own arrays and mp_thompson_batch converts.
  subroutine mp_thompson_staging(ncol, nz, st, fo, pp, ok)
    integer, intent(in) :: ncol, nz
    real, pointer, intent(out) :: st(:,:,:), fo(:,:,:), pp(:,:)
    logical, intent(out) :: ok
    integer(c_size_t) :: nprof, esize
    nullify(st, fo, pp)
    ok = (kind(1.0) == c_double .and. trim(kidmp_arith) == 'p64') .or. &
         (kind(1.0) == c_float .and. trim(kidmp_arith) /= 'p64')
    if (.not. ok) return
    nprof = int(nz, c_size_t) * int(ncol, c_size_t)
    esize = int(storage_size(1.0) / 8, c_size_t)
    call staging(1, esize * 12 * nprof);  call staging(2, esize * 3 * nprof);  call staging(3, esize * 4 * ncol)
    call c_f_pointer(hbuf(1), st, [nz, ncol, 12]);  call c_f_pointer(hbuf(2), fo, [nz, ncol, 3]);  call c_f_pointer(hbuf(3), pp, [4, ncol])
  end subroutine mp_thompson_staging

  ! ncol columns in one launch.  Arrays are (nz, ncol), k fastest -- KiD's own
  ! storage order -- and ppt is (4, ncol) = rain, snow, graupel, ice, accumulated.
  ! What KiD never fills may be left out (keyword call): nc, nwfa, nifa and w without is_aerosol_aware (W:36 passes
  ! them unset; the library forms the non-aerosol defaults of M:958-964 on the GPU), qi, qs, qg, ni in an iiwarm run
  ! (they stay zero, W:46-52).  Absent arrays are neither staged nor sent across PCIe.
  subroutine mp_thompson_batch(ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, dbz, &
       re_qc, re_qi, re_qs)
    integer, intent(in) :: ncol, nz
    real, intent(in) :: dt
    real, dimension(nz,ncol), intent(inout), target :: qv, qc, qr, nr, t
    real, dimension(nz,ncol), intent(inout), optional, target :: qi, qs, qg, ni, nc, nwfa, nifa
    real, dimension(nz,ncol), intent(in), target :: p, dz
    real, dimension(nz,ncol), intent(in), optional, target :: w
    real, dimension(4,ncol), intent(inout), target :: ppt
    ! dbz (optional): calc_refl10cm (M:4946-5244) of the post-step state, formed on the GPU in the same host call
    real, dimension(nz,ncol), intent(out), optional, target :: dbz
    ! re_qc, re_qi, re_qs (optional, all three): calc_effectRad (M:4834-4935) of the post-step state in the form of the
    ! scheme's driver -- presets first, M:1111-1116 --, formed by the same launch as dbz (kidmp_batch_step_host_out)
    real, dimension(nz,ncol), intent(out), optional, target :: re_qc, re_qi, re_qs
    real(c_double), pointer :: rates(:,:,:)
    integer(c_int32_t), pointer :: nstep(:,:)
    type(kidmp_outputs) :: out
    type(c_ptr) :: prates, pnstep, ps(15)
    integer(c_size_t) :: nprof, esize
    integer(c_int) :: rc
    logical :: have_frz, have_aer, want_radii, is64, inplace
    integer :: i, n
    if (.not. c_associated(ctx)) call thompson_init
    have_frz = present(qi);  have_aer = present(nc)
    if ((have_frz .neqv. present(qs)) .or. (have_frz .neqv. present(qg)) .or. (have_frz .neqv. present(ni)) .or. &
        (have_aer .neqv. present(nwfa)) .or. (have_aer .neqv. present(nifa))) then
       write(*,'(a)') ' module_mp_thompson09n: qi, qs, qg, ni (and nc, nwfa, nifa) must be passed or left out together'
       stop 1
    end if
    want_radii = present(re_qc)
    call radii_together(want_radii, present(re_qi), present(re_qs))
    if ((present(dbz) .or. want_radii) .and. c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: radar reflectivity is not available with kidmp_ndevices > 1'
       stop 1
    end if
    ! ---- the storage kind of the staging arrays: binary64 for 'p64' (a 4-byte REAL is converted on the way), else
    !      binary32 state straight to the GPU: the reference's own REAL / DOUBLE PRECISION split, or all binary32 ----
    is64 = trim(kidmp_arith) == 'p64'
    if (.not. is64 .and. kind(qv) /= c_float) then
       write(*,'(3a)') ' module_mp_thompson09n: kidmp_arith=', trim(kidmp_arith), ' needs KiD built with 4-byte default REAL'
       stop 1
    end if
    esize = merge(8_c_size_t, 4_c_size_t, is64)
    n = nz * ncol
    nprof = int(nz, c_size_t) * int(ncol, c_size_t)
    call rate_staging(ncol, nz, rates, nstep, prates, pnstep)
    call staging(1, esize * 12 * nprof);  call staging(2, esize * 3 * nprof);  call staging(3, esize * 4 * ncol)
    do i = 1, 12                                           ! the slots: 1..12 the state, 13..15 p, w, dz
       ps(i) = byte_offset(hbuf(1), (i - 1) * esize * nprof)
    end do
    do i = 1, 3
       ps(12 + i) = byte_offset(hbuf(2), (i - 1) * esize * nprof)
    end do
    ! (an argument that IS its staging slot -- mp_thompson_staging -- needs no copy, in or out)
    inplace = c_associated(c_loc(qv), ps(1)) .and. c_associated(c_loc(qc), ps(2)) .and. c_associated(c_loc(qr), ps(4)) .and. &
         c_associated(c_loc(nr), ps(8)) .and. c_associated(c_loc(t), ps(12)) .and. c_associated(c_loc(p), ps(13)) .and. &
         c_associated(c_loc(dz), ps(15)) .and. c_associated(c_loc(ppt), hbuf(3))
    if (inplace .and. have_frz) inplace = c_associated(c_loc(qi), ps(3)) .and. c_associated(c_loc(qs), ps(5)) .and. &
         c_associated(c_loc(qg), ps(6)) .and. c_associated(c_loc(ni), ps(7))
    if (inplace .and. have_aer) inplace = c_associated(c_loc(nc), ps(9)) .and. c_associated(c_loc(nwfa), ps(10)) .and. &
         c_associated(c_loc(nifa), ps(11))
    if (inplace .and. present(w)) inplace = c_associated(c_loc(w), ps(14))
    if (.not. inplace) then
       call put(ps(1), qv, n);  call put(ps(2), qc, n);  call put(ps(4), qr, n);  call put(ps(8), nr, n);  call put(ps(12), t, n)
       if (have_frz) then
          call put(ps(3), qi, n);  call put(ps(5), qs, n);  call put(ps(6), qg, n);  call put(ps(7), ni, n)
       end if
       if (have_aer) then
          call put(ps(9), nc, n);  call put(ps(10), nwfa, n);  call put(ps(11), nifa, n)
       end if
       call put(ps(13), p, n);  call put(ps(15), dz, n)
       if (present(w)) call put(ps(14), w, n)
       call put(hbuf(3), ppt, 4 * ncol)
    end if
    ! absent arrays are not sent: the library sees NULL
    if (.not. have_frz) then
       ps(3) = c_null_ptr;  ps(5:7) = c_null_ptr
    end if
    if (.not. have_aer) ps(9:11) = c_null_ptr
    if (.not. present(w)) ps(14) = c_null_ptr
    out = kidmp_outputs(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz) .or. want_radii) then                 ! one GPU, the step followed by ONE launch for the outputs
       call staging(6, esize * 4 * nprof)
       if (present(dbz)) out%dbz = hbuf(6)
       if (want_radii) then
          out%re_qc = byte_offset(hbuf(6), esize * nprof);  out%re_qi = byte_offset(hbuf(6), 2 * esize * nprof)
          out%re_qs = byte_offset(hbuf(6), 3 * esize * nprof)
       end if
    end if
    if (.not. is64) then
       rc = kidmp32_batch_step_host_out(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), real(dt, c_float), &
            ps(1), ps(2), ps(3), ps(4), ps(5), ps(6), ps(7), ps(8), ps(9), ps(10), ps(11), ps(12), &
            ps(13), ps(14), ps(15), hbuf(3), prates, pnstep, arith_code(), out)
    else if (c_associated(mctx)) then                      ! several GPUs: contiguous column ranges, one pipeline each
       rc = kidmp_batch_step_host_multi(mctx, int(ncol, c_int64_t), int(nz, c_int32_t), real(dt, c_double), &
            ps(1), ps(2), ps(3), ps(4), ps(5), ps(6), ps(7), ps(8), ps(9), ps(10), ps(11), ps(12), &
            ps(13), ps(14), ps(15), hbuf(3), prates, pnstep, kidmp_precip_sums)
    else
       rc = kidmp_batch_step_host_out(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), real(dt, c_double), &
            ps(1), ps(2), ps(3), ps(4), ps(5), ps(6), ps(7), ps(8), ps(9), ps(10), ps(11), ps(12), &
            ps(13), ps(14), ps(15), hbuf(3), prates, pnstep, out)
    end if
    call stop_on_error(rc, 'mp_thompson')
    if (present(dbz)) call get(out%dbz, dbz, n)
    if (want_radii) then
       call get(out%re_qc, re_qc, n);  call get(out%re_qi, re_qi, n);  call get(out%re_qs, re_qs, n)
    end if
    if (.not. inplace) then
       call get(ps(1), qv, n);  call get(ps(2), qc, n);  call get(ps(4), qr, n);  call get(ps(8), nr, n);  call get(ps(12), t, n)
       if (have_frz) then
          call get(ps(3), qi, n);  call get(ps(5), qs, n);  call get(ps(6), qg, n);  call get(ps(7), ni, n)
       end if
       if (have_aer) then
          call get(ps(9), nc, n);  call get(ps(10), nwfa, n);  call get(ps(11), nifa, n)
       end if
       call get(hbuf(3), ppt, 4 * ncol)
    end if
    if (l_rate_diagnostics) call replay_rate_diagnostics(ncol, nz, rates, nstep)

  contains

    ! m values of the caller's REAL to / from staging memory of the arithmetic's storage kind
    subroutine put(slot, a, m)
      type(c_ptr), intent(in) :: slot
      integer, intent(in) :: m
      real, intent(in) :: a(m)
      real(c_double), pointer :: v8(:)
      real(c_float), pointer :: v4(:)
      if (is64) then
         call c_f_pointer(slot, v8, [m]);  v8 = a
      else
         call c_f_pointer(slot, v4, [m]);  v4 = a
      end if
    end subroutine put

    subroutine get(slot, a, m)
      type(c_ptr), intent(in) :: slot
      integer, intent(in) :: m
      real, intent(out) :: a(m)
      real(c_double), pointer :: v8(:)
      real(c_float), pointer :: v4(:)
      if (is64) then
         call c_f_pointer(slot, v8, [m]);  a = real(v8)
      else
         call c_f_pointer(slot, v4, [m]);  a = v4
      end if
    end subroutine get
  end subroutine mp_thompson_batch

  ! The KiD block of M:2962-3124: per column, per level, 30 mixed-phase rates (.not. iiwarm) then 6 warm ones;
  ! save_dg(k, value, ...) when nx == 1, save_dg(k, ii, value, ...) otherwise; a column that left through the no_micro
  ! return (M:1540: all four substep counts 0) never reached the block.
  subroutine replay_rate_diagnostics(ncol, nz, rates, nstep)
    integer, intent(in) :: ncol, nz
    real(c_double), intent(in) :: rates(nz, NRATES, ncol)
    integer(c_int32_t), intent(in) :: nstep(4, ncol)
    integer :: i, k, r, r0
    r0 = 1
    if (iiwarm) r0 = NRATES_MIXED + 1
    do i = 1, ncol
       if (all(nstep(:,i) == 0)) cycle
       do k = 1, nz
          do r = r0, NRATES
             if (nx == 1) then
                call save_dg(k, rates(k,r,i), rate_names(r), i_dgtime, units='/kg/s', dim='z')
             else
                call save_dg(k, i, rates(k,r,i), rate_names(r), i_dgtime, units='/kg/s', dim='z')
             end if
          end do
       end do
    end do
  end subroutine replay_rate_diagnostics

  ! Page-locked work arrays for a caller of mp_thompson_kid_interface whose hydrometeor moments are not plain arrays
  ! (KiD keeps them in a derived type): hyd(nz,ncol,7,4) = the moments qc, qr, nr, qi, ni, qs, qg of the state, of the
  ! advective and of the divergence tendencies (IN) and of the microphysics tendencies (OUT); pp(4,ncol).
  subroutine mp_thompson_kid_staging(ncol, nz, hyd, pp)
    integer, intent(in) :: ncol, nz
    real, pointer, intent(out) :: hyd(:,:,:,:), pp(:,:)
    integer(c_size_t) :: esize
    esize = int(storage_size(1.0) / 8, c_size_t)
    call staging(7, esize * 28 * int(nz, c_size_t) * int(ncol, c_size_t));  call staging(3, esize * 4 * ncol)
    call c_f_pointer(hbuf(7), hyd, [nz, ncol, 7, 4]);  call c_f_pointer(hbuf(3), pp, [4, ncol])
  end subroutine mp_thompson_kid_staging

  ! mphys_thompson09_interfacen (W:28-310) in ONE library call: KiD's theta-form fields and their advective and divergence
  ! tendencies in, the microphysics tendencies and the surface precipitation out; the gather (W:59-97) and the back-out
  ! (W:198-245) run on the GPU beside the step (kidmp_kid_interface_host, kidmp32_* for 4-byte default REAL).  Arrays are
  ! (nz, ncol); hyd* carry the moments qc, qr, nr, qi, ni, qs, qg (the last four are not looked at in an iiwarm run);
  ! dz is KiD's one profile; ppt is (4, ncol) = rain, snow, graupel, ice, OUT.  dbz, re_*: as mp_thompson_batch.
  ! The arrays go to the library as they are: no copy, no conversion -- so the build's REAL must be what kidmp_arith
  ! stores (8-byte with 'p64', 4-byte with 'p32n' / 'f32').
  subroutine mp_thompson_kid_interface(ncol, nz, dt, p0, r_on_cp, theta, qv, hyd, dtheta_adv, dqv_adv, hyd_adv, &
       dtheta_div, dqv_div, hyd_div, exner, dz, dtheta_mphys, dqv_mphys, hyd_mphys, ppt, dbz, re_qc, re_qi, re_qs)
    integer, intent(in) :: ncol, nz
    real, intent(in) :: dt, p0, r_on_cp
    real, dimension(nz,ncol), intent(in), target :: theta, qv, dtheta_adv, dqv_adv, dtheta_div, dqv_div, exner
    real, dimension(nz,ncol,7), intent(in), target :: hyd, hyd_adv, hyd_div
    real, dimension(nz), intent(in), target :: dz
    real, dimension(nz,ncol), intent(out), target :: dtheta_mphys, dqv_mphys
    real, dimension(nz,ncol,7), intent(inout), target :: hyd_mphys
    real, dimension(4,ncol), intent(out), target :: ppt
    real, dimension(nz,ncol), intent(out), optional, target :: dbz, re_qc, re_qi, re_qs
    type(kidmp_kid_fields) :: state, adv, div, mphys
    type(kidmp_outputs) :: out
    real(c_double), pointer :: rates(:,:,:)
    integer(c_int32_t), pointer :: nstep(:,:)
    type(c_ptr) :: prates, pnstep
    integer(c_int) :: rc
    integer :: n
    if (.not. c_associated(ctx)) call thompson_init
    if (c_associated(mctx)) then
       write(*,'(a)') ' module_mp_thompson09n: mp_thompson_kid_interface is not available with kidmp_ndevices > 1'
       stop 1
    end if
    if ((kind(theta) == c_double) .neqv. (trim(kidmp_arith) == 'p64')) then
       write(*,'(3a)') ' module_mp_thompson09n: mp_thompson_kid_interface with kidmp_arith=', trim(kidmp_arith), &
            ' needs the matching default REAL (8-byte for p64, 4-byte for p32n / f32)'
       stop 1
    end if
    call radii_together(present(re_qc), present(re_qi), present(re_qs))
    n = nz * ncol
    state = kid_fields(n, theta, qv, hyd);  adv = kid_fields(n, dtheta_adv, dqv_adv, hyd_adv)
    div = kid_fields(n, dtheta_div, dqv_div, hyd_div);  mphys = kid_fields(n, dtheta_mphys, dqv_mphys, hyd_mphys)
    out = kidmp_outputs(c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
    if (present(dbz)) out%dbz = c_loc(dbz)
    if (present(re_qc)) then
       out%re_qc = c_loc(re_qc);  out%re_qi = c_loc(re_qi);  out%re_qs = c_loc(re_qs)
    end if
    call rate_staging(ncol, nz, rates, nstep, prates, pnstep)
    if (kind(theta) == c_double) then
       rc = kidmp_kid_interface_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), real(dt, c_double), real(p0, c_double), &
            real(r_on_cp, c_double), state, adv, div, c_loc(exner), c_loc(dz), mphys, c_loc(ppt), prates, pnstep, out)
    else
       rc = kidmp32_kid_interface_host(ctx, int(ncol, c_int64_t), int(nz, c_int32_t), real(dt, c_float), real(p0, c_float), &
            real(r_on_cp, c_float), state, adv, div, c_loc(exner), c_loc(dz), mphys, c_loc(ppt), prates, pnstep, out, arith_code())
    end if
    call stop_on_error(rc, 'mp_thompson_kid_interface')
    if (l_rate_diagnostics) call replay_rate_diagnostics(ncol, nz, rates, nstep)
  end subroutine mp_thompson_kid_interface

end module module_mp_thompson09n
