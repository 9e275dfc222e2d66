! Test driver of column_summary_batch through the Fortran drop-in (kid_amd/fortran/module_mp_thompson09n.f90), built against
! the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in build/, 4 bytes in build32/).
!
!   kid_summary_driver FILE [full | warm | cfg DBZ_ECHO Q_CLOUD T_FREEZE]
!       FILE = "nz ncol", then nz lines "dz", then ncol*nz lines "t p qv qc nc qi qr nr qs qg", column after column, kts first.
!       full: a mixed-phase run, every optional array is passed (the default); warm: an iiwarm run, the arguments from nc on
!       are left out; cfg: as full with the three thresholds passed.  Prints "SUM i s value" for the 16 slots s of column i.
program kid_summary_driver
  use iso_c_binding, only: c_double
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: column_summary_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: mode, arg
  integer :: n, ncol, i, k, u, s
  real, allocatable, dimension(:,:) :: t, p, qv, qc, nc, qi, qr, nr, qs, qg
  real, allocatable :: dz(:)
  real(c_double), allocatable :: summary(:,:)
  real :: thr(3)

  call get_command_argument(1, path)
  mode = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, mode)
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qc(n,ncol), nc(n,ncol), qi(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), &
       qg(n,ncol), dz(n), summary(16,ncol))
  do k = 1, n
     read(u, *) dz(k)
  end do
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qc(k,i), nc(k,i), qi(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i)
     end do
  end do
  close(u)
  iiwarm = trim(mode) == 'warm'
  if (trim(mode) == 'warm') then
     call column_summary_batch(ncol, n, t, p, qv, qc, qr, nr, dz, summary)
  else if (trim(mode) == 'cfg') then
     do s = 1, 3
        call get_command_argument(2 + s, arg);  read(arg, *) thr(s)
     end do
     call column_summary_batch(ncol, n, t, p, qv, qc, qr, nr, dz, summary, nc, qi, qs, qg, thr(1), thr(2), thr(3))
  else
     call column_summary_batch(ncol, n, t, p, qv, qc, qr, nr, dz, summary, nc, qi, qs, qg)
  end if
  do i = 1, ncol
     do s = 1, 16
        write(*, '(a,2i6,es26.17e3)') 'SUM', i, s - 1, summary(s,i)
     end do
  end do
  call thompson_finalize
end program kid_summary_driver
