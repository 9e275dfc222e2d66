! Test driver of calc_effectRad through the Fortran drop-in (kid_amd/fortran/*.f90), built against the KiD stand-ins of
! kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_effrad_driver FILE
!       calc_effectRad on one column.  FILE = "nz" then nz lines "t p qv qc nc qi ni qs re_qc re_qi re_qs" (kts first; the
!       last three are the values the INOUT radii hold before the call).  Prints "RE k re_qc re_qi re_qs".
!   kid_effrad_driver batch FILE [full | nonc | warm]
!       calc_effectRad_batch on several columns.  FILE = "nz ncol" then ncol*nz lines as above, column after column.
!       nonc: nc is left out of the call; warm: an iiwarm run, nc, qi, ni and qs are left out.  Prints "RE k i ...".
!   kid_effrad_driver adapter nx case refl radii [arith [aero]]
!       one call of mphys_thompson09_interfacen on nx columns (case warm | mixed, the soundings of kid_mini_driver) with
!       mphys_thompson09n's l_radar_reflectivity = (refl == 1) and l_effective_radii = (radii == 1),
!       module_mp_thompson09n's kidmp_arith = arith (p64 default) and is_aerosol_aware = (aero == 1); every save_dg call
!       is recorded to dg_dump.txt, and post_state.txt receives per column and level the post-step state the library
!       returned (t p qv qc nc qi ni qr nr qs qg, read from the staging arrays the adapter stepped in place; what the
!       call left out is written as zero) followed by dtheta_mphys and dqv_mphys.
program kid_effrad_driver
  use parameters, only: nz, nx
  use column_variables
  use namelists, only: iiwarm, set_Nc
  use diagnostics, only: recording, nlog, dump_log
  use mphys_thompson09n, only: mphys_thompson09_interfacen, l_radar_reflectivity, l_effective_radii
  use module_mp_thompson09n, only: calc_effectRad, calc_effectRad_batch, thompson_finalize, mp_thompson_staging, &
       kidmp_arith, is_aerosol_aware
  implicit none
  character(1024) :: arg1, path
  character(64) :: arg, which

  call get_command_argument(1, arg1)
  if (trim(arg1) == 'adapter') then
     call adapter_run()
  else if (trim(arg1) == 'batch') then
     call get_command_argument(2, path)
     arg = 'full'
     if (command_argument_count() >= 3) call get_command_argument(3, arg)
     call batch_run(trim(path), trim(arg))
  else
     call column_run(trim(arg1))
  end if
  call thompson_finalize

contains

  subroutine column_run(file)
    character(*), intent(in) :: file
    integer :: n, k, u
    real, allocatable, dimension(:) :: t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs
    open(newunit=u, file=file, status='old', action='read')
    read(u, *) n
    allocate(t(n), p(n), qv(n), qc(n), nc(n), qi(n), ni(n), qs(n), re_qc(n), re_qi(n), re_qs(n))
    do k = 1, n
       read(u, *) t(k), p(k), qv(k), qc(k), nc(k), qi(k), ni(k), qs(k), re_qc(k), re_qi(k), re_qs(k)
    end do
    close(u)
    call calc_effectRad(t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs, 1, n)
    do k = 1, n
       write(*, '(a,i6,3es26.17)') 'RE', k, re_qc(k), re_qi(k), re_qs(k)
    end do
  end subroutine column_run

  subroutine batch_run(file, mode)
    character(*), intent(in) :: file, mode
    integer :: n, ncol, i, k, u
    real, allocatable, dimension(:,:) :: t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs
    open(newunit=u, file=file, status='old', action='read')
    read(u, *) n, ncol
    allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qc(n,ncol), nc(n,ncol), qi(n,ncol), ni(n,ncol), qs(n,ncol), &
         re_qc(n,ncol), re_qi(n,ncol), re_qs(n,ncol))
    do i = 1, ncol
       do k = 1, n
          read(u, *) t(k,i), p(k,i), qv(k,i), qc(k,i), nc(k,i), qi(k,i), ni(k,i), qs(k,i), re_qc(k,i), re_qi(k,i), re_qs(k,i)
       end do
    end do
    close(u)
    if (mode == 'warm') then
       iiwarm = .true.
       call calc_effectRad_batch(ncol, n, t, p, qv, qc, re_qc, re_qi, re_qs)
    else if (mode == 'nonc') then
       call calc_effectRad_batch(ncol, n, t, p, qv, qc, re_qc, re_qi, re_qs, qi=qi, ni=ni, qs=qs)
    else
       call calc_effectRad_batch(ncol, n, t, p, qv, qc, re_qc, re_qi, re_qs, nc, qi, ni, qs)
    end if
    do i = 1, ncol
       do k = 1, n
          write(*, '(a,2i6,3es26.17)') 'RE', k, i, re_qc(k,i), re_qi(k,i), re_qs(k,i)
       end do
    end do
  end subroutine batch_run

  subroutine adapter_run()
    integer :: i, k
    real :: z, p, t, es, qsat
    real, pointer :: st(:,:,:), fo(:,:,:), pp(:,:)
    double precision :: frz(4), anc
    logical :: ok
    call get_command_argument(2, arg);  read(arg, *) nx
    call get_command_argument(3, which)
    call get_command_argument(4, arg);  l_radar_reflectivity = trim(arg) == '1'
    call get_command_argument(5, arg);  l_effective_radii = trim(arg) == '1'
    if (command_argument_count() >= 6) call get_command_argument(6, kidmp_arith)
    if (command_argument_count() >= 7) then
       call get_command_argument(7, arg);  is_aerosol_aware = trim(arg) == '1'
    end if
    iiwarm = trim(which) /= 'mixed';  set_Nc = 100.0
    call alloc_columns(nz, nx)
    do i = 1, nx
       do k = 1, nz
          if (iiwarm) then                     ! the KiD warm-rain sounding of kid_mini_driver
             z = (k-0.5)*25.
             dz(k) = 25.
             p = 1.e5*(1.-2.2557e-5*z)**5.2559
             exner(k,i) = (p/1.e5)**(287.058/1005.)
             t = 297. - 6.5e-3*z
             theta(k,i) = t/exner(k,i)
             qv(k,i) = 0.015 - 0.004*z/3000.
             if (z > 800. .and. z < 2000.) then
                hydrometeors(k,i,1)%moments(1,1) = 8.e-4
                hydrometeors(k,i,2)%moments(1,1) = 3.e-4*(1. + 0.2*(i-1))
                hydrometeors(k,i,2)%moments(1,2) = 2.e4
             end if
          else                                 ! the mixed-phase deep-convection sounding of kid_mini_driver
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
    recording = .true.
    nlog = 0
    call mphys_thompson09_interfacen
    call dump_log('dg_dump.txt')
    ! the post-step state: the adapter steps the library's staging arrays in place (mp_thompson_staging)
    call mp_thompson_staging(nx, nz, st, fo, pp, ok)
    if (.not. ok) then
       write(*,'(a)') ' kid_effrad_driver: the default REAL does not match kidmp_arith (no staging arrays to read)'
       stop 3
    end if
    open(23, file='post_state.txt', status='replace')
    do i = 1, nx
       do k = 1, nz
          frz = 0.d0;  anc = 0.d0              ! left out of the call: a warm run's frozen species, nc without aerosols
          if (.not. iiwarm .or. is_aerosol_aware) frz = (/ dble(st(k,i,3)), dble(st(k,i,7)), dble(st(k,i,5)), dble(st(k,i,6)) /)
          if (is_aerosol_aware) anc = dble(st(k,i,9))
          write(23, '(13es25.17)') dble(st(k,i,12)), dble(fo(k,i,1)), dble(st(k,i,1)), dble(st(k,i,2)), anc, frz(1), frz(2), &
               dble(st(k,i,4)), dble(st(k,i,8)), frz(3), frz(4), dble(dtheta_mphys(k,i)), dble(dqv_mphys(k,i))
       end do
    end do
    close(23)
  end subroutine adapter_run

end program kid_effrad_driver
