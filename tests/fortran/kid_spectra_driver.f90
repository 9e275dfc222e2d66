! The size spectra through the Fortran drop-in (kid_amd/fortran): size_spectra_batch of module_mp_thompson09n, built
! against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
! The complete example.
!
!   kid_spectra_driver FILE [warm]
!       FILE = "nz ncol nb", then nb lines "D dD" (a grid for rain; nb = 0: the scheme's own), then ncol*nz lines
!       "t p qv qc nc qi ni qr nr qs qg", column after column, kts first.  Every parameter and every spectrum are asked
!       for, rain on the grid of the file and the others on the scheme's own 100 bins; warm: an iiwarm run, nc, qi, ni,
!       qs and qg are left out.  Prints "PAR name i k value" for every parameter and "BIN x i b k value" for every bin.
program kid_spectra_driver
  use iso_c_binding, only: c_double
  use namelists, only: iiwarm, set_Nc
  use module_mp_thompson09n, only: size_spectra_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, nb, nbr, i, k, b, u, v
  real, allocatable, dimension(:,:) :: t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg
  real, allocatable :: par(:,:,:), n_c(:,:,:), n_i(:,:,:), n_r(:,:,:), n_s(:,:,:), n_g(:,:,:)
  real(c_double), allocatable :: D(:), dD(:)
  character(5), parameter :: names(11) = (/ 'lam_c', 'n0_c ', 'nu_c ', 'lam_i', 'n0_i ', 'lam_r', 'n0_r ', 'smob ', 'smoc ', &
       'lam_g', 'n0_g ' /)
  logical :: warm

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_spectra_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol, nb
  nbr = nb
  if (nb == 0) nbr = 100
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qc(n,ncol), nc(n,ncol), qi(n,ncol), ni(n,ncol), qr(n,ncol), nr(n,ncol), &
       qs(n,ncol), qg(n,ncol), par(n,ncol,11), n_c(n,100,ncol), n_i(n,100,ncol), n_r(n,nbr,ncol), n_s(n,100,ncol), &
       n_g(n,100,ncol), D(nb), dD(nb))
  do b = 1, nb
     read(u, *) D(b), dD(b)
  end do
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qc(k,i), nc(k,i), qi(k,i), ni(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i)
     end do
  end do
  close(u)
  iiwarm = warm;  set_Nc = 100.0
  if (warm) then
     call size_spectra_batch(ncol, n, t, p, qv, qc, qr, nr, n_c, n_i, n_r, n_s, n_g, par(:,:,1), par(:,:,2), par(:,:,3), &
          par(:,:,4), par(:,:,5), par(:,:,6), par(:,:,7), par(:,:,8), par(:,:,9), par(:,:,10), par(:,:,11))
  else if (nb > 0) then
     call size_spectra_batch(ncol, n, t, p, qv, qc, qr, nr, n_c, n_i, n_r, n_s, n_g, par(:,:,1), par(:,:,2), par(:,:,3), &
          par(:,:,4), par(:,:,5), par(:,:,6), par(:,:,7), par(:,:,8), par(:,:,9), par(:,:,10), par(:,:,11), &
          nc=nc, qi=qi, ni=ni, qs=qs, qg=qg, D_r=D, dD_r=dD)
  else
     call size_spectra_batch(ncol, n, t, p, qv, qc, qr, nr, n_c, n_i, n_r, n_s, n_g, par(:,:,1), par(:,:,2), par(:,:,3), &
          par(:,:,4), par(:,:,5), par(:,:,6), par(:,:,7), par(:,:,8), par(:,:,9), par(:,:,10), par(:,:,11), &
          nc=nc, qi=qi, ni=ni, qs=qs, qg=qg)
  end if
  do v = 1, 11
     do i = 1, ncol
        do k = 1, n
           write(*, '(a,1x,a,2i6,es26.17e3)') 'PAR', trim(names(v)), i, k, par(k,i,v)
        end do
     end do
  end do
  call dump('c', n_c)
  call dump('i', n_i)
  call dump('r', n_r)
  call dump('s', n_s)
  call dump('g', n_g)
  call thompson_finalize

contains

  subroutine dump(x, a)
    character(1), intent(in) :: x
    real, intent(in) :: a(:,:,:)
    integer :: ii, bb, kk
    do ii = 1, size(a, 3)
       do bb = 1, size(a, 2)
          do kk = 1, size(a, 1)
             write(*, '(a,1x,a,3i6,es26.17e3)') 'BIN', x, ii, bb, kk, a(kk,bb,ii)
          end do
       end do
    end do
  end subroutine dump
end program kid_spectra_driver
