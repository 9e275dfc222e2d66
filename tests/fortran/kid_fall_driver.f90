! The fall speeds through the Fortran drop-in (kid_amd/fortran): fall_speeds_batch of module_mp_thompson09n and the adapter's
! l_precip_flux, built against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/,
! 4 bytes in build32/).  The complete example of both.
!
!   kid_fall_driver batch FILE [warm]
!       FILE = "nz ncol dt", then nz lines "dz", then ncol*nz lines "t p qv qr nr qi ni qs qg boost", column after column,
!       kts first.  Every output and nstep are asked for; warm: an iiwarm run, qi, ni, qs, qg and vts_boost are left out.
!       Prints "FALL name i k value" for every profile and "NSTEP i r i s g" for every column.
!   kid_fall_driver kid NX NSTEPS CASE DUMP_STEP FLUX [NDEVICES]
!       The step loop of kid_mini_driver on its case (warm | mixed, zero forcing) with l_precip_flux = FLUX (0 | 1): the
!       save_dg calls of step DUMP_STEP go to dg_dump.txt, and the state the adapter left after that step (its staging
!       arrays: T, p, qv, qr, nr, qi, ni, qs, qg per level) to post_state.txt.  NDEVICES: module_mp_thompson09n's
!       kidmp_ndevices (devices 0 .. NDEVICES-1).
program kid_fall_driver
  use iso_c_binding, only: c_int32_t
  use parameters, only: nz, nx, dt
  use column_variables
  use namelists, only: iiwarm, set_Nc
  use diagnostics, only: recording, nlog, dump_log
  use mphys_thompson09n, only: mphys_thompson09_interfacen, l_precip_flux
  use module_mp_thompson09n, only: fall_speeds_batch, mp_thompson_staging, thompson_finalize, kidmp_ndevices, &
       kidmp_devices
  implicit none
  character(1024) :: path
  character(64) :: mode, arg, which

  call get_command_argument(1, mode)
  if (trim(mode) == 'batch') then
     call get_command_argument(2, path)
     arg = 'full'
     if (command_argument_count() >= 3) call get_command_argument(3, arg)
     call run_batch(trim(path), trim(arg) == 'warm')
  else if (trim(mode) == 'kid') then
     call run_kid
  else
     write(*,'(a)') ' kid_fall_driver: batch FILE [warm] | kid NX NSTEPS CASE DUMP_STEP FLUX [NDEVICES]'
     stop 2
  end if
  call thompson_finalize

contains

  subroutine run_batch(file, warm)
    character(*), intent(in) :: file
    logical, intent(in) :: warm
    integer :: n, ncol, i, k, u, v
    real :: step
    real, allocatable, dimension(:,:) :: t, p, qv, qr, nr, qi, ni, qs, qg, boost
    real, allocatable :: o(:,:,:), dzc(:)
    integer(c_int32_t), allocatable :: nstep(:,:)
    character(10), parameter :: names(11) = (/ 'vt_r      ', 'vt_nr     ', 'vt_i      ', 'vt_ni     ', 'vt_s      ', 'vt_g      ', &
         'flux_r    ', 'flux_i    ', 'flux_s    ', 'flux_g    ', 'flux_total' /)
    open(newunit=u, file=file, status='old', action='read')
    read(u, *) n, ncol, step
    allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qr(n,ncol), nr(n,ncol), qi(n,ncol), ni(n,ncol), qs(n,ncol), qg(n,ncol), &
         boost(n,ncol), o(n,ncol,11), dzc(n), nstep(4,ncol))
    do k = 1, n
       read(u, *) dzc(k)
    end do
    do i = 1, ncol
       do k = 1, n
          read(u, *) t(k,i), p(k,i), qv(k,i), qr(k,i), nr(k,i), qi(k,i), ni(k,i), qs(k,i), qg(k,i), boost(k,i)
       end do
    end do
    close(u)
    iiwarm = warm
    if (warm) then
       call fall_speeds_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
            o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), dz=dzc, dt=step, nstep=nstep)
    else
       call fall_speeds_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
            o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), qi=qi, ni=ni, qs=qs, qg=qg, vts_boost=boost, dz=dzc, dt=step, nstep=nstep)
    end if
    do v = 1, 11
       do i = 1, ncol
          do k = 1, n
             write(*, '(a,1x,a,2i6,es26.17e3)') 'FALL', trim(names(v)), i, k, o(k,i,v)
          end do
       end do
    end do
    do i = 1, ncol
       write(*, '(a,5i8)') 'NSTEP', i, nstep(:,i)
    end do
  end subroutine run_batch

  subroutine run_kid
    integer :: k, i, n, j, nsteps, dump_step
    real :: z, p, t, es, qsat
    real, pointer :: st(:,:,:), fo(:,:,:), ppt(:,:)
    logical :: staged
    call get_command_argument(2, arg); read(arg,*) nx
    call get_command_argument(3, arg); read(arg,*) nsteps
    call get_command_argument(4, which)
    call get_command_argument(5, arg); read(arg,*) dump_step
    call get_command_argument(6, arg)
    l_precip_flux = trim(arg) == '1'
    if (command_argument_count() >= 7) then
       call get_command_argument(7, arg); read(arg,*) kidmp_ndevices
       do i = 1, kidmp_ndevices
          kidmp_devices(i) = i - 1
       end do
    end if
    iiwarm = trim(which) /= 'mixed'; set_Nc = 100.0
    call alloc_columns(nz, nx)
    do i = 1, nx                                   ! the cases of kid_mini_driver, statement for statement
       do k = 1, nz
          if (iiwarm) then
             z = (k-0.5)*25.
             dz(k) = 25.
             p = 1.e5*(1.-2.2557e-5*z)**5.2559
             exner(k,i) = (p/1.e5)**(287.058/1005.)
             t = 297. - 6.5e-3*z
             theta(k,i) = t/exner(k,i)
             qv(k,i) = 0.015 - 0.004*z/3000.
             if (z > 800. .and. z < 2000.) then
                hydrometeors(k,i,1)%moments(1,1) = 8.e-4
                hydrometeors(k,i,2)%moments(1,1) = 3.e-4
                hydrometeors(k,i,2)%moments(1,2) = 2.e4
             end if
          else
             z = (k-0.5)*125.
             dz(k) = 125.
             p = 1.e5*(1.-2.2557e-5*z)**5.2559
             exner(k,i) = (p/1.e5)**(287.058/1005.)
             t = max(210., 300. - 6.5e-3*z)
             theta(k,i) = t/exner(k,i)
             es = 611.2*exp(17.67*(t-273.15)/(t-29.65))
             qsat = 0.622*es/(p-es)
             qv(k,i) = 0.7*qsat
             if (z > 1000. .and. z < 4000.) then
                qv(k,i) = 1.02*qsat
                hydrometeors(k,i,1)%moments(1,1) = 1.e-3
                hydrometeors(k,i,2)%moments(1,1) = 5.e-4
                hydrometeors(k,i,2)%moments(1,2) = 5.e3
             else if (z > 4000. .and. z < 11000.) then
                qv(k,i) = qsat
                hydrometeors(k,i,1)%moments(1,1) = 2.e-4
                hydrometeors(k,i,2)%moments(1,1) = 1.e-4
                hydrometeors(k,i,2)%moments(1,2) = 1.e3
                hydrometeors(k,i,3)%moments(1,1) = 1.e-4
                hydrometeors(k,i,3)%moments(1,2) = 1.e5
                hydrometeors(k,i,4)%moments(1,1) = 1.e-3
                hydrometeors(k,i,5)%moments(1,1) = 2.e-3
             end if
             hydrometeors(k,i,2)%moments(1,1) = hydrometeors(k,i,2)%moments(1,1)*(1. + 0.1*(i-1))
          end if
       end do
    end do
    do n = 1, nsteps
       recording = n == dump_step
       if (recording) nlog = 0
       call mphys_thompson09_interfacen
       if (recording) then
          call dump_log('dg_dump.txt')
          ! what the adapter stepped: the library's staging arrays in the order of mp_thompson's arguments
          ! (qv qc qi qr qs qg ni nr nc nwfa nifa t; p is fo(:,:,1)), untouched since the call
          call mp_thompson_staging(nx, nz, st, fo, ppt, staged)
          if (staged) then
             open(24, file='post_state.txt', status='replace')
             do i = 1, nx
                do k = 1, nz
                   if (iiwarm) then
                      write(24,'(9es26.17e3)') st(k,i,12), fo(k,i,1), st(k,i,1), st(k,i,4), st(k,i,8), 0., 0., 0., 0.
                   else
                      write(24,'(9es26.17e3)') st(k,i,12), fo(k,i,1), st(k,i,1), st(k,i,4), st(k,i,8), st(k,i,3), st(k,i,7), &
                           st(k,i,5), st(k,i,6)
                   end if
                end do
             end do
             close(24)
          end if
       end if
       theta = theta + dt*(dtheta_mphys + dtheta_adv + dtheta_div)
       qv = qv + dt*(dqv_mphys + dqv_adv + dqv_div)
       do j = 1, 5
          do i = 1, nx
             do k = 1, nz
                hydrometeors(k,i,j)%moments = hydrometeors(k,i,j)%moments + dt*(dhydrometeors_mphys(k,i,j)%moments &
                     + dhydrometeors_adv(k,i,j)%moments + dhydrometeors_div(k,i,j)%moments)
             end do
          end do
       end do
    end do
  end subroutine run_kid
end program kid_fall_driver
