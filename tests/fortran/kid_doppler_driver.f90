! The radar moments through the Fortran drop-in (kid_amd/fortran): doppler_moments_batch of module_mp_thompson09n, built
! against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_doppler_driver FILE [warm]
!       FILE = "nz ncol", then ncol*nz lines "t p qv qr nr qs qg w", column after column, kts first.  Every output is
!       asked for; warm: an iiwarm run, and the optional qs, qg and w are left out.
!       Prints "DOPPLER name i k value" for every profile.
program kid_doppler_driver
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: doppler_moments_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, i, k, u, v
  logical :: warm
  real, allocatable, dimension(:,:) :: t, p, qv, qr, nr, qs, qg, w
  real, allocatable :: o(:,:,:)
  character(5), parameter :: names(9) = (/ 'dbz  ', 'vd   ', 'sw   ', 'vz_r ', 'vz_s ', 'vz_g ', 'dbz_r', 'dbz_s', 'dbz_g' /)

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_doppler_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), qg(n,ncol), w(n,ncol), o(n,ncol,9))
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i), w(k,i)
     end do
  end do
  close(u)
  iiwarm = warm
  if (warm) then
     call doppler_moments_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
          o(:,:,8), o(:,:,9))
  else
     call doppler_moments_batch(ncol, n, t, p, qv, qr, nr, o(:,:,1), o(:,:,2), o(:,:,3), o(:,:,4), o(:,:,5), o(:,:,6), o(:,:,7), &
          o(:,:,8), o(:,:,9), qs=qs, qg=qg, w=w)
  end if
  do v = 1, 9
     do i = 1, ncol
        do k = 1, n
           write(*, '(a,1x,a,2i6,es26.17e3)') 'DOPPLER', trim(names(v)), i, k, o(k,i,v)
        end do
     end do
  end do
  call thompson_finalize
end program kid_doppler_driver
