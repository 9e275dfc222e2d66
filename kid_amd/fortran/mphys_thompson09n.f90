!
! mphys_thompson09n -- KiD-facing adapter of the MI355X Thompson-09n build.
!
! Drop-in for the reference adapter of the same name (/root/reference/mphys_thompson09n.f90, "W:"): same module
! name, same public entry `mphys_thompson09_interfacen` without arguments, data exchanged through KiD's own
! modules (parameters, column_variables, physconst, namelists, diagnostics; W:11-17), same results:
!   * d*_mphys tendencies = (state after microphysics - state)/dt - forcing          (W:198-245)
!   * surface precipitation diagnostics through save_dg, in the reference's order     (W:155-182, W:248-303)
!
! Design differences (see INTEGRATION.md):
!   * the reference loops `do i=1,nx` over one-column mp_thompson calls (W:54-246); here the nx columns are
!     packed once into a (nz, nx, slot) work array -- k fastest, KiD's own order, which is also the layout of the
!     C ABI -- and advanced by ONE batched call (one GPU launch);
!   * species are handled by a small slot table instead of one hand-written statement per species;
!   * the inputs the reference passes unset (nc1d, nwfa1d, nifa1d, w1d; W:36) get the scheme's non-aerosol
!     defaults (module_mp_thompson09n.f90 of the reference, lines 958-964).
!
module mphys_thompson09n

  Use parameters, only : num_h_moments, num_h_bins, nspecies, nz, dt &
       , h_names, mom_units, max_char_len, nx
  Use column_variables
  Use physconst, only : p0, r_on_cp, pi
  Use namelists, only : iiwarm, set_Nc
  Use module_mp_thompson09n
  Use diagnostics, only: save_dg, i_dgtime

  Implicit None

  ! public module variables of the reference adapter (W:22-24)
  logical :: micro_unset=.True.
  ! calc_refl10cm (M:4946-5244) of the post-step state, asked for in the same host call and saved as 'dBZ' (z,x) after
  ! the precipitation diagnostics.  .false.: call sequence and output as without it.
  logical, public :: l_radar_reflectivity = .false.
  ! calc_effectRad (M:4834-4935) of the post-step state in the form of the scheme's driver (presets first, M:1111-1116),
  ! asked for in the same host call and saved as 're_cloud', 're_ice', 're_snow' (the driver's names, M:1118-1120; m,
  ! z,x) at the end of the sequence, after 'dBZ' if that is on too.  .false.: call sequence and output as without it.
  logical, public :: l_effective_radii = .false.
  ! A droplet number per column, cm**-3 like the namelist's set_Nc (M:22): allocated with size nx, column i is stepped with
  ! Nt_c = set_Nc_column(i)*1.e6 (M:381) -- a stock 2-D case then has x as the axis of an Nd ensemble, all members in
  ! one launch.  Unallocated: call sequence and results as without it.  Any other size stops the run.
  real, allocatable, public :: set_Nc_column(:)
  ! .true.: the gather (W:59-97) and the back-out (W:198-245) run on the GPU inside the one library call
  ! (mp_thompson_kid_interface): theta, exner, qv and their forcing arrays go to the library as they are, only the
  ! derived-type hydrometeor moments are copied into work arrays and scattered back, and the two arithmetic loops below
  ! are not run.  Needs one device, and a default REAL that is what kidmp_arith stores.  .false.: call sequence and
  ! results as without it.
  logical, public :: l_device_adapter = .false.
  ! .true. (nx > 1): 'total_ppt_level' carries dt * flux_total of the post-step state, kg m-2 per step like pptrain --
  ! the sedimentation flux v*rho*q of rain + ice + snow + graupel across every level (fall_speeds_batch, one more host
  ! call per step) -- in the place of the zeros of U6; name, units string and dim='z,x' are unchanged.  Needs one device
  ! and the host-side adapter (not l_device_adapter, which leaves no post-step state on the host).  .false.: call
  ! sequence, save_dg sequence and every result as without it.
  logical, public :: l_precip_flux = .false.
  real, allocatable, private, save :: nc_bound(:)          ! what is bound in the library (unallocated: nothing)
  integer:: ih, imom
  character(max_char_len) :: name, units

  ! slots of the packed state, in the argument order of mp_thompson / the C ABI
  integer, parameter, private :: S_QV=1, S_QC=2, S_QI=3, S_QR=4, S_QS=5, S_QG=6, S_NI=7, S_NR=8, &
       S_NC=9, S_NWFA=10, S_NIFA=11, S_T=12, NSLOT=12
  ! prognostic hydrometeor moments KiD carries for this scheme: (state slot, KiD species, KiD moment)
  ! KiD species: 1 cloud, 2 rain, 3 ice, 4 snow, 5 graupel; moment 1 mass, 2 number (W:66-93)
  integer, parameter, private :: NHYD = 7
  integer, parameter, private :: hyd_slot(NHYD) = (/ S_QC, S_QR, S_NR, S_QI, S_NI, S_QS, S_QG /)
  integer, parameter, private :: hyd_spec(NHYD) = (/ 1,    2,    2,    3,    3,    4,    5    /)
  integer, parameter, private :: hyd_mom (NHYD) = (/ 1,    1,    2,    1,    2,    1,    1    /)
  ! precipitation diagnostics in the reference's call order rain, ice, snow, graupel (W:158-177):
  ! KiD species index and row of ppt(4,:) = (rain, snow, graupel, ice)
  integer, parameter, private :: dg_spec(4) = (/ 2, 3, 4, 5 /)
  integer, parameter, private :: dg_row (4) = (/ 1, 4, 2, 3 /)

contains

  Subroutine mphys_thompson09_interfacen

    ! Work arrays: the library's page-locked staging arrays themselves where KiD's REAL is what the selected arithmetic
    ! stores (mp_thompson_staging; no copy between here and PCIe), else heap arrays kept between calls (as automatic
    ! arrays they overflow the stack from nx ~ 500 on).  pres, wvel, dzc are fo(:,:,1:3).
    real, pointer :: st(:,:,:), fo(:,:,:), ppt(:,:)
    real, pointer :: hy(:,:,:,:)                             ! l_device_adapter: (nz, nx, 7, 4) = state, adv, div, mphys
    real, allocatable, target, save :: st_own(:,:,:), fo_own(:,:,:), ppt_own(:,:)
    real, allocatable, save :: total(:)
    real, allocatable, save :: pptrain_2d_prof(:,:)          ! W:32; saved as 'total_ppt_level' for nx > 1 (W:304-307)
    real, allocatable, save :: dbz(:,:)                      ! l_radar_reflectivity: (nz, nx)
    real, allocatable, target, save :: re(:,:,:)             ! l_effective_radii: (nz, nx, 3) = cloud water, ice, snow
    ! the optional arguments of the one batched call: a disassociated pointer is an absent argument, and `contiguous`
    ! lets an associated one pass without a temporary, so that the library still finds a staging slot to be itself
    real, pointer, contiguous :: o_qi(:,:), o_qs(:,:), o_qg(:,:), o_ni(:,:), o_nc(:,:), o_nwfa(:,:), o_nifa(:,:), o_w(:,:)
    real, pointer, contiguous :: o_rc(:,:), o_ri(:,:), o_rs(:,:)
    real :: rho
    logical :: staged
    integer :: i, k, m, s

    if (l_precip_flux) then                      ! refused before anything is initialised
       if (kidmp_ndevices > 1) then
          write(*,'(a)') ' mphys_thompson09n: l_precip_flux is not available with kidmp_ndevices > 1'
          stop 1
       end if
       if (l_device_adapter) then
          write(*,'(a)') ' mphys_thompson09n: l_precip_flux is not available with l_device_adapter'
          stop 1
       end if
    end if
    if (micro_unset) then                        ! W:100-103 (ahead of the gather: the staging arrays belong to the library)
       call thompson_init
       micro_unset = .False.
    end if
    if (l_device_adapter) then
       if (kidmp_ndevices > 1) then
          write(*,'(a)') ' mphys_thompson09n: l_device_adapter is not available with kidmp_ndevices > 1'
          stop 1
       end if
       call mp_thompson_kid_staging(nx, nz, hy, ppt)
       staged = .true.
    else
       call mp_thompson_staging(nx, nz, st, fo, ppt, staged)
    end if
    if (.not. staged) then
       if (allocated(st_own)) then
          if (size(st_own,1) /= nz .or. size(st_own,2) /= nx) deallocate(st_own, fo_own, ppt_own)
       end if
       if (.not. allocated(st_own)) allocate(st_own(nz,nx,NSLOT), fo_own(nz,nx,3), ppt_own(4,nx))
       st => st_own;  fo => fo_own;  ppt => ppt_own
    end if
    if (allocated(total)) then
       if (size(total) /= nx) deallocate(total)
    end if
    if (.not. allocated(total)) allocate(total(nx))

    if (.not. l_device_adapter) then
    ! ---- gather: state + (advective + divergence forcing)*dt, W:59-97 ----
    ! Columns are independent: the loop over i is shared among OpenMP threads when the model is built with OpenMP
    ! (the directives are comments otherwise).  At nx = 10^4 this host-side packing, not the GPU, bounds a KiD step.
    !$omp parallel do default(shared) private(i, k, m, s) schedule(static) if(nx >= 256)
    do i = 1, nx
       st(:,i,S_T)  = (theta(:,i) + (dtheta_adv(:,i) + dtheta_div(:,i))*dt)*exner(:,i)
       fo(:,i,1)    = p0*exner(:,i)**(1./r_on_cp)
       fo(:,i,3)    = dz(:)
       st(:,i,S_QV) = qv(:,i) + (dqv_adv(:,i) + dqv_div(:,i))*dt
       do m = 1, NHYD
          if (iiwarm .and. hyd_spec(m) > 2) cycle
          s = hyd_slot(m)
          do k = 1, nz
             st(k,i,s) = hydrometeors(k,i,hyd_spec(m))%moments(1,hyd_mom(m)) &
                  + (dhydrometeors_adv(k,i,hyd_spec(m))%moments(1,hyd_mom(m)) &
                  +  dhydrometeors_div(k,i,hyd_spec(m))%moments(1,hyd_mom(m)))*dt
          end do
       end do
    end do
    !$omp end parallel do
    ! What the reference leaves unset (nc1d, nwfa1d, nifa1d, w1d; W:36): with is_aerosol_aware they are read, and get
    ! the scheme's non-aerosol defaults (M:958-964) and no updraft here; without it they are left out of the call and
    ! the library forms the same defaults on the GPU, so they never cross PCIe.
    if (is_aerosol_aware) then
       fo(:,:,2) = 0.0
       if (iiwarm) then
          ! a warm run keeps qc1d..qg1d at their initial zeros (W:46-52): the aerosol-aware call below passes all
          ! twelve slots, and the staging memory is neither zeroed by the library nor by ALLOCATE
          st(:,:,S_QI) = 0.0;  st(:,:,S_QS) = 0.0;  st(:,:,S_QG) = 0.0;  st(:,:,S_NI) = 0.0
       end if
       do i = 1, nx
          do k = 1, nz
             rho = 0.622*fo(k,i,1)/(287.04*st(k,i,S_T)*(st(k,i,S_QV)+0.622))
             st(k,i,S_NC)   = set_Nc*1.e6/rho
             st(k,i,S_NWFA) = 11.1E6/rho
             st(k,i,S_NIFA) = 0.5E6*0.01/rho
          end do
       end do
    end if
    end if

    ! ---- the droplet number per column: bound before the batched call, again only when its contents changed ----
    if (allocated(set_Nc_column)) then
       if (size(set_Nc_column) /= nx) then
          write(*,'(a,i0,a,i0)') ' mphys_thompson09n: set_Nc_column has ', size(set_Nc_column), ' elements, nx = ', nx
          stop 1
       end if
       if (allocated(nc_bound)) then
          if (size(nc_bound) /= nx) deallocate(nc_bound)
       end if
       if (.not. allocated(nc_bound)) then
          allocate(nc_bound(nx))
          nc_bound = set_Nc_column
          call mp_thompson_set_column_nc(nc_bound)
       else if (any(nc_bound /= set_Nc_column)) then
          nc_bound = set_Nc_column
          call mp_thompson_set_column_nc(nc_bound)
       end if
    else if (allocated(nc_bound)) then                      ! deallocated since the last call: back to the namelist's set_Nc
       deallocate(nc_bound)
       call mp_thompson_set_column_nc()
    end if

    ! ---- all nx columns in one call (replaces the loop around W:143-152) ----
    if (.not. l_device_adapter) ppt = 0.0
    if (allocated(dbz)) then
       if (size(dbz, 1) /= nz .or. size(dbz, 2) /= nx .or. .not. l_radar_reflectivity) deallocate(dbz)
    end if
    if (l_radar_reflectivity .and. .not. allocated(dbz)) allocate(dbz(nz, nx))
    if (l_effective_radii) then
       if (allocated(re)) then
          if (size(re, 1) /= nz .or. size(re, 2) /= nx) deallocate(re)
       end if
       if (.not. allocated(re)) allocate(re(nz, nx, 3))
    end if
    ! What goes to the library beside the always-present arrays.  dbz is allocated only with l_radar_reflectivity: an
    ! unallocated actual argument is an absent optional one, like a disassociated pointer.  The frozen species of a warm
    ! run stay zero (W:46-52) and stay at home; the aerosols and w are sent only where they are read.
    nullify(o_qi, o_qs, o_qg, o_ni, o_nc, o_nwfa, o_nifa, o_w, o_rc, o_ri, o_rs)
    if (l_effective_radii) then
       o_rc => re(:,:,1);  o_ri => re(:,:,2);  o_rs => re(:,:,3)
    end if
    if (.not. l_device_adapter .and. (is_aerosol_aware .or. .not. iiwarm)) then
       o_qi => st(:,:,S_QI);  o_qs => st(:,:,S_QS);  o_qg => st(:,:,S_QG);  o_ni => st(:,:,S_NI)
    end if
    if (.not. l_device_adapter .and. is_aerosol_aware) then
       o_nc => st(:,:,S_NC);  o_nwfa => st(:,:,S_NWFA);  o_nifa => st(:,:,S_NIFA);  o_w => fo(:,:,2)
    end if
    if (l_device_adapter) then
       ! ---- gather, step and back-out in one library call: only the derived-type moments are copied ----
       !$omp parallel do default(shared) private(i, k, m) schedule(static) if(nx >= 256)
       do i = 1, nx
          do m = 1, NHYD
             if (iiwarm .and. hyd_spec(m) > 2) cycle
             do k = 1, nz
                hy(k,i,m,1) = hydrometeors(k,i,hyd_spec(m))%moments(1,hyd_mom(m))
                hy(k,i,m,2) = dhydrometeors_adv(k,i,hyd_spec(m))%moments(1,hyd_mom(m))
                hy(k,i,m,3) = dhydrometeors_div(k,i,hyd_spec(m))%moments(1,hyd_mom(m))
             end do
          end do
       end do
       !$omp end parallel do
       call mp_thompson_kid_interface(nx, nz, dt, p0, r_on_cp, theta(:,1:nx), qv(:,1:nx), hy(:,:,:,1), &
            dtheta_adv(:,1:nx), dqv_adv(:,1:nx), hy(:,:,:,2), dtheta_div(:,1:nx), dqv_div(:,1:nx), hy(:,:,:,3), &
            exner(:,1:nx), dz, dtheta_mphys(:,1:nx), dqv_mphys(:,1:nx), hy(:,:,:,4), ppt, dbz, o_rc, o_ri, o_rs)
       !$omp parallel do default(shared) private(i, k, m) schedule(static) if(nx >= 256)
       do i = 1, nx
          do m = 1, NHYD
             if (iiwarm .and. hyd_spec(m) > 2) cycle
             do k = 1, nz
                dhydrometeors_mphys(k,i,hyd_spec(m))%moments(1,hyd_mom(m)) = hy(k,i,m,4)
             end do
          end do
       end do
       !$omp end parallel do
    else
       call mp_thompson_batch(nx, nz, dt, st(:,:,S_QV), st(:,:,S_QC), o_qi, st(:,:,S_QR), o_qs, o_qg, o_ni, st(:,:,S_NR), &
            o_nc, o_nwfa, o_nifa, st(:,:,S_T), fo(:,:,1), o_w, fo(:,:,3), ppt, dbz, o_rc, o_ri, o_rs)
    end if

    if (.not. l_device_adapter) then
    ! ---- back out the microphysics tendencies, W:198-245 ----
    !$omp parallel do default(shared) private(i, k, m, s) schedule(static) if(nx >= 256)
    do i = 1, nx
       dtheta_mphys(:,i) = (st(:,i,S_T)/exner(:,i) - theta(:,i))/dt - (dtheta_adv(:,i) + dtheta_div(:,i))
       dqv_mphys(:,i)    = (st(:,i,S_QV) - qv(:,i))/dt - (dqv_adv(:,i) + dqv_div(:,i))
       do m = 1, NHYD
          if (iiwarm .and. hyd_spec(m) > 2) cycle
          s = hyd_slot(m)
          do k = 1, nz
             dhydrometeors_mphys(k,i,hyd_spec(m))%moments(1,hyd_mom(m)) = &
                  (st(k,i,s) - hydrometeors(k,i,hyd_spec(m))%moments(1,hyd_mom(m)))/dt &
                  - (dhydrometeors_adv(k,i,hyd_spec(m))%moments(1,hyd_mom(m)) &
                  +  dhydrometeors_div(k,i,hyd_spec(m))%moments(1,hyd_mom(m)))
          end do
       end do
    end do
    !$omp end parallel do
    end if

    ! ---- surface precipitation diagnostics ----
    imom = 1
    units = trim(mom_units(imom))//' m'
    total = ppt(4,:) + ppt(1,:) + ppt(2,:) + ppt(3,:)          ! ice + rain + snow + graupel, as W:181
    if (nx == 1) then                                          ! W:155-182
       do m = 1, 4
          ih = dg_spec(m)
          name = 'surface_ppt_for_'//trim(h_names(ih))
          call save_dg(ppt(dg_row(m),1), name, i_dgtime, units, dim='time')
       end do
       name = 'total_surface_ppt'
       call save_dg(total(1)/nx, name, i_dgtime, units, dim='time')
    else                                                       ! W:248-303: domain means, then every column
       do m = 1, 4
          ih = dg_spec(m)
          name = 'surface_ppt_for_'//trim(h_names(ih))
          call save_dg(ppt(dg_row(m),:)/nx, name, i_dgtime, units, dim='time')
       end do
       name = 'total_surface_ppt'
       call save_dg(total/nx, name, i_dgtime, units, dim='time')
       do m = 1, 4
          ih = dg_spec(m)
          name = 'surface_ppt_for_'//trim(h_names(ih))
          call save_dg(ppt(dg_row(m),:), name, i_dgtime, units, dim='time')
       end do
       name = 'total_surface_ppt'
       call save_dg(total, name, i_dgtime, units, dim='time')
       ! save precip flux at all levels and columns, W:304-307.  The reference saves pptrain_2d_prof(nz,nx), an array it
       ! never assigns (W:191 is commented out), i.e. undefined values under a name every stock KiD output carries.
       ! Defined semantics here (U6): the name, units, dim='z,x' and shape of the reference, all values zero.
       ! With l_precip_flux the array is assigned at last: dt * flux_total of the post-step state (cf. M:3395, W:191).
       if (allocated(pptrain_2d_prof)) then
          if (size(pptrain_2d_prof, 1) /= nz .or. size(pptrain_2d_prof, 2) /= nx) deallocate(pptrain_2d_prof)
       end if
       if (.not. allocated(pptrain_2d_prof)) then
          allocate(pptrain_2d_prof(nz, nx))
          pptrain_2d_prof = 0.0
       end if
       if (l_precip_flux) then
          if (iiwarm) then
             call fall_speeds_batch(nx, nz, st(:,:,S_T), fo(:,:,1), st(:,:,S_QV), st(:,:,S_QR), st(:,:,S_NR), &
                  flux_total=pptrain_2d_prof)
          else
             call fall_speeds_batch(nx, nz, st(:,:,S_T), fo(:,:,1), st(:,:,S_QV), st(:,:,S_QR), st(:,:,S_NR), &
                  flux_total=pptrain_2d_prof, qi=st(:,:,S_QI), ni=st(:,:,S_NI), qs=st(:,:,S_QS), qg=st(:,:,S_QG))
          end if
          pptrain_2d_prof = dt*pptrain_2d_prof
       else
          pptrain_2d_prof = 0.0
       end if
       name = 'total_ppt_level'
       call save_dg(pptrain_2d_prof, name, i_dgtime, units, dim='z,x')
    end if
    ! ---- radar reflectivity (calc_refl10cm of the post-step state; no bright band, as the reference ships it) ----
    if (l_radar_reflectivity) call save_dg(dbz, 'dBZ', i_dgtime, 'dBZ', dim='z,x')
    ! ---- effective radii for radiation coupling (calc_effectRad of the post-step state) ----
    if (l_effective_radii) then
       call save_dg(re(:,:,1), 're_cloud', i_dgtime, 'm', dim='z,x')
       call save_dg(re(:,:,2), 're_ice', i_dgtime, 'm', dim='z,x')
       call save_dg(re(:,:,3), 're_snow', i_dgtime, 'm', dim='z,x')
    end if

  end Subroutine mphys_thompson09_interfacen

end module mphys_thompson09n
