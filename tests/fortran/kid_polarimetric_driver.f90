! The polarimetric radar through the Fortran drop-in (kid_amd/fortran): polarimetric_batch of module_mp_thompson09n, built
! against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_polarimetric_driver FILE [warm]
!       FILE = "nz ncol", then "wavelength eps_w_re eps_w_im eps_i_re eps_i_im rho_w rho_i", then
!       "axis_r(1..5) axis_r_min axis_s axis_g sigma(1..3) force_quadrature", then ncol*nz lines "t p qv qr nr qs qg",
!       column after column, kts first.  Every output is asked for; warm: an iiwarm run, and every optional argument but the
!       outputs is left out (the defaults of the library).
!       Prints "POL name i k value" for every profile.
program kid_polarimetric_driver
  use, intrinsic :: iso_c_binding, only: c_double
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: polarimetric_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, i, k, u, v, fq
  logical :: warm
  real(c_double) :: c(7), a(11)
  real, allocatable, dimension(:,:) :: t, p, qv, qr, nr, qs, qg
  real, allocatable :: o(:,:,:)
  character(8), parameter :: names(13) = (/ 'dbz_h   ', 'zdr     ', 'kdp     ', 'rhohv   ', 'dbz_h_r ', 'dbz_h_s ', 'dbz_h_g ', &
       'zdr_r   ', 'zdr_s   ', 'zdr_g   ', 'kdp_r   ', 'kdp_s   ', 'kdp_g   ' /)

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_polarimetric_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol
  read(u, *) c
  read(u, *) a, fq
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), qg(n,ncol))
  allocate(o(n,ncol,13))
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i)
     end do
  end do
  close(u)
  iiwarm = warm
  if (warm) then
     call polarimetric_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
          o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), o(:,:,12), o(:,:,13))
  else
     call polarimetric_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
          o(:,:,8), o(:,:,9), o(:,:,10), o(:,:,11), o(:,:,12), o(:,:,13), qs=qs, qg=qg, wavelength=c(1), eps_w_re=c(2), &
          eps_w_im=c(3), eps_i_re=c(4), eps_i_im=c(5), rho_w=c(6), rho_i=c(7), axis_r=a(1:5), axis_r_min=a(6), axis_s=a(7), &
          axis_g=a(8), sigma=a(9:11), force_quadrature=fq /= 0)
  end if
  do v = 1, 13
     do i = 1, ncol
        do k = 1, n
           write(*, '(a,1x,a,2i6,es26.17e3)') 'POL', trim(names(v)), i, k, o(k,i,v)
        end do
     end do
  end do
  call thompson_finalize
end program kid_polarimetric_driver
