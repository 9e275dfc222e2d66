! The Doppler spectrum through the Fortran drop-in (kid_amd/fortran): doppler_spectrum_batch of module_mp_thompson09n, built
! against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_dspectrum_driver FILE [warm]
!       FILE = "nz ncol nv v0 dv nbs", then nbs lines "D dD" (a diameter grid for snow; nbs = 0: the scheme's own bins),
!       then ncol*nz lines "t p qv qr nr qs qg w", column after column, kts first.  Every output is asked for; warm: an
!       iiwarm run, and the optional qs, qg, w and grid are left out.
!       Prints "DSPEC name i k j value" for every spectrum (j the velocity bin) and, with j = 0, for below and above.
program kid_dspectrum_driver
  use, intrinsic :: iso_c_binding, only: c_double
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: doppler_spectrum_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, nv, nbs, i, k, j, u, v
  logical :: warm
  real(c_double) :: v0, dv
  real(c_double), allocatable :: D(:), dD(:)
  real, allocatable, dimension(:,:) :: t, p, qv, qr, nr, qs, qg, w
  real, allocatable :: s(:,:,:,:), e(:,:,:)
  character(7), parameter :: names(6) = (/ 'total  ', 'rain   ', 'snow   ', 'graupel', 'below  ', 'above  ' /)

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_dspectrum_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol, nv, v0, dv, nbs
  allocate(D(nbs), dD(nbs))
  do k = 1, nbs
     read(u, *) D(k), dD(k)
  end do
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), qg(n,ncol), w(n,ncol))
  allocate(s(n,nv,ncol,4), e(n,ncol,2))
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i), w(k,i)
     end do
  end do
  close(u)
  iiwarm = warm
  if (warm) then
     call doppler_spectrum_batch(ncol, n, t, p, qv, qr, nr, v0, dv, nv, s(:,:,:,1), s(:,:,:,2), s(:,:,:,3), s(:,:,:,4), &
          e(:,:,1), e(:,:,2))
  else if (nbs > 0) then
     call doppler_spectrum_batch(ncol, n, t, p, qv, qr, nr, v0, dv, nv, s(:,:,:,1), s(:,:,:,2), s(:,:,:,3), s(:,:,:,4), &
          e(:,:,1), e(:,:,2), qs=qs, qg=qg, w=w, D_s=D, dD_s=dD)
  else
     call doppler_spectrum_batch(ncol, n, t, p, qv, qr, nr, v0, dv, nv, s(:,:,:,1), s(:,:,:,2), s(:,:,:,3), s(:,:,:,4), &
          e(:,:,1), e(:,:,2), qs=qs, qg=qg, w=w)
  end if
  do v = 1, 4
     do i = 1, ncol
        do j = 1, nv
           do k = 1, n
              write(*, '(a,1x,a,3i6,es26.17e3)') 'DSPEC', trim(names(v)), i, k, j, s(k,j,i,v)
           end do
        end do
     end do
  end do
  do v = 1, 2
     do i = 1, ncol
        do k = 1, n
           write(*, '(a,1x,a,3i6,es26.17e3)') 'DSPEC', trim(names(v + 4)), i, k, 0, e(k,i,v)
        end do
     end do
  end do
  call thompson_finalize
end program kid_dspectrum_driver
