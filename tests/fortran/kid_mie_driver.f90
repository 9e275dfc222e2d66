! The cloud radar through the Fortran drop-in (kid_amd/fortran): mie_radar_batch of module_mp_thompson09n, built against the
! KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_mie_driver FILE [warm]
!       FILE = "nz ncol", then "wavelength eps_w_re eps_w_im eps_i_re eps_i_im rho_w rho_i kw2", then nz lines "dz k_gas",
!       then ncol*nz lines "t p qv qc qr nr qs qg w", column after column, kts first.  Every output is asked for; warm: an
!       iiwarm run, and the optional qc, qs, qg, w, k_gas, rho_w, rho_i and kw2 are left out.
!       Prints "MIE name i k value" for every profile and "MIE pia_total i 0 value" for the column's attenuation.
program kid_mie_driver
  use, intrinsic :: iso_c_binding, only: c_double
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: mie_radar_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, i, k, u, v
  logical :: warm
  real(c_double) :: c(8)
  real, allocatable, dimension(:,:) :: t, p, qv, qc, qr, nr, qs, qg, w
  real, allocatable :: dz(:), k_gas(:), o(:,:,:), pia(:)
  character(8), parameter :: names(13) = (/ 'dbz     ', 'dbz_up  ', 'dbz_down', 'dbz_r   ', 'dbz_s   ', 'dbz_g   ', 'mie_r   ', &
       'mie_s   ', 'mie_g   ', 'ext     ', 'pia_up  ', 'pia_down', 'vd      ' /)

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_mie_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol
  read(u, *) c
  allocate(dz(n), k_gas(n))
  do k = 1, n
     read(u, *) dz(k), k_gas(k)
  end do
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qc(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), qg(n,ncol), w(n,ncol))
  allocate(o(n,ncol,13), pia(ncol))
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qc(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i), w(k,i)
     end do
  end do
  close(u)
  iiwarm = warm
  if (warm) then
     call mie_radar_batch(ncol, n, c(1), c(2), c(3), c(4), c(5), t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), &
          o(:,:,5), o(:,:,6), o(:,:,7), o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), o(:,:,12), o(:,:,13), pia, dz=dz)
  else
     call mie_radar_batch(ncol, n, c(1), c(2), c(3), c(4), c(5), t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), &
          o(:,:,5), o(:,:,6), o(:,:,7), o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), o(:,:,12), o(:,:,13), pia, qc=qc, qs=qs, &
          qg=qg, dz=dz, w=w, k_gas=k_gas, rho_w=c(6), rho_i=c(7), kw2=c(8))
  end if
  do v = 1, 13
     do i = 1, ncol
        do k = 1, n
           write(*, '(a,1x,a,2i6,es26.17e3)') 'MIE', trim(names(v)), i, k, o(k,i,v)
        end do
     end do
  end do
  do i = 1, ncol
     write(*, '(a,1x,a,2i6,es26.17e3)') 'MIE', 'pia_total', i, 0, pia(i)
  end do
  call thompson_finalize
end program kid_mie_driver
