! Driver of the REFERENCE Fortran (module_mp_thompson09n.f90 / mphys_thompson09n.f90 compiled in place from $(REF), see
! oracle/Makefile, target `ref`), linked against the KiD stand-ins of tests/fortran/kid_stubs.f90.  Test infrastructure:
! tests/golden/make_reference_goldens.py runs it to record what the Fortran itself computes.
!
!   ref_driver IN OUT        (run with the tree as working directory: the reference opens run_data/... relative to it)
!
! IN and OUT are little-endian stream files.  `real` below is the default REAL of the tree (8 bytes in _ref/p64, 4 bytes
! in _ref/native); everything written to OUT is binary64 whatever the tree.
!   IN  header: int32 mode (1 step, 2 tables, 3 adapter), int32 iiwarm, int32 l_sediment, int32 bytes of a real (checked),
!               real64 set_Nc, real64 dt
!   mode 1, blocks until ncol = 0:
!       IN   int32 ncol, int32 nz, int32 is_aerosol_aware, then qv qc qi qr qs qg ni nr nc nwfa nifa t p w dz, each
!            real [nz, ncol] (level fastest)
!       OUT  the 12 stepped profiles in that order [nz, ncol, 12]; ppt rain, snow, graupel, ice [4, ncol]; the 36 rates of
!            the save_dg log [nz, 36, ncol] (a rate the call did not log stays 0); dBZ of calc_refl10cm and re_qc, re_qi,
!            re_qs of calc_effectRad on the stepped state [nz, ncol, 4], then the same on the input state
!   mode 2:  OUT for each table of `tables` below: int32 rank, int32 dims(4), the values; then the 16 public t?_q?_?? scalars
!   mode 3:  IN   int32 nx, int32 nz, real64 p0, real64 r_on_cp, then real theta, dtheta_adv, dtheta_div, exner [nz, nx],
!                 dz [nz], qv, dqv_adv, dqv_div [nz, nx], hydrometeors, dhydrometeors_adv, dhydrometeors_div [nz, nx, 5, 2]
!            OUT  dtheta_mphys, dqv_mphys [nz, nx], dhydrometeors_mphys [nz, nx, 5, 2], int32 nlog, then per log entry
!                 character(8) form, character(40) name, int32 k, int32 i, real64 value
program ref_driver
  use parameters, only: nz, nx, dt
  use switches, only: l_sediment, l_reuse_thompson_lookup
  use namelists, only: iiwarm, set_Nc
  use physconst, only: p0, r_on_cp
  use diagnostics, only: recording, nlog, log_name, log_form, log_k, log_i, log_v
  use column_variables
  use module_mp_thompson09n
  use mphys_thompson09n, only: mphys_thompson09_interfacen
  implicit none
  integer, parameter :: nrates = 36
  character(7), parameter :: rate_names(nrates) = (/ &
       'pri_inu', 'pri_ide', 'prs_ide', 'prs_sde', 'prg_gde', 'pri_wfz', 'prs_scw', 'prg_scw', 'prg_gcw', &
       'pri_ihm', 'pri_rfz', 'prs_iau', 'prs_sci', 'pri_rci', 'pni_inu', 'pni_ihm', 'pni_wfz', 'pni_rfz', &
       'pni_ide', 'pni_iau', 'pni_sci', 'pni_rci', 'prr_sml', 'prr_gml', 'pnr_rcs', 'pnr_rcg', 'pnr_rci', &
       'pnr_sml', 'pnr_gml', 'pnr_rfz', 'prr_wau', 'prr_rcw', 'prv_rev', 'pnr_wau', 'pnr_rev', 'pnr_rcr' /)
  character(1024) :: fin, fout
  integer :: uin, uout, mode, iw, ised, rbytes
  double precision :: nc64, dt64
  real :: probe

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=uin, file=trim(fin), access='stream', form='unformatted', status='old', action='read')
  open(newunit=uout, file=trim(fout), access='stream', form='unformatted', status='replace', action='write')
  read(uin) mode, iw, ised, rbytes, nc64, dt64
  if (rbytes /= storage_size(probe)/8) stop 'ref_driver: IN was written for the other tree (size of a real)'
  iiwarm = iw /= 0;  l_sediment = ised /= 0;  set_Nc = real(nc64);  dt = real(dt64)
  l_reuse_thompson_lookup = .true.
  if (mode == 3) then
     call adapter_mode()
  else
     nx = 1
     call thompson_init
     if (mode == 1) call step_mode()
     if (mode == 2) call tables_mode()
  end if
  close(uin);  close(uout)

contains

  subroutine step_mode()
    integer :: ncol, n, aero, c, j, k, m
    real, allocatable :: a(:,:,:), b(:,:,:)
    double precision, allocatable :: ppt(:,:), rates(:,:,:), diag(:,:,:,:)
    real :: pr, ps, pg, pi
    do
       read(uin) ncol, n, aero
       if (ncol <= 0) exit
       is_aerosol_aware = aero /= 0
       allocate(a(n,ncol,15), b(n,ncol,15), ppt(4,ncol), rates(n,nrates,ncol), diag(n,ncol,4,2))
       read(uin) a
       b = a
       rates = 0.d0
       do c = 1, ncol
          nlog = 0;  recording = .true.
          pr = 0.;  ps = 0.;  pg = 0.;  pi = 0.
          call mp_thompson(b(:,c,1), b(:,c,2), b(:,c,3), b(:,c,4), b(:,c,5), b(:,c,6), b(:,c,7), b(:,c,8), b(:,c,9), &
               b(:,c,10), b(:,c,11), b(:,c,12), b(:,c,13), b(:,c,14), b(:,c,15), pr, ps, pg, pi, 1, n, dt, 1, 1)
          recording = .false.
          ppt(:,c) = (/ dble(pr), dble(ps), dble(pg), dble(pi) /)
          do m = 1, nlog
             if (log_form(m) /= 'k') cycle
             do j = 1, nrates
                if (trim(log_name(m)) == rate_names(j)) rates(log_k(m), j, c) = log_v(m)
             end do
          end do
          call diagnose(b(:,c,:), n, diag(:,c,:,1))
          call diagnose(a(:,c,:), n, diag(:,c,:,2))
       end do
       write(uout) dble(b(:,:,1:12)), ppt, rates, diag
       deallocate(a, b, ppt, rates, diag)
    end do
  end subroutine step_mode

  ! calc_refl10cm and calc_effectRad on one column s(:, 1:15); the radii start from the presets of the 3-D driver
  subroutine diagnose(s, n, d)
    integer, intent(in) :: n
    real, intent(in) :: s(n,15)
    double precision, intent(out) :: d(n,4)
    real :: dbz(n), rc(n), ri(n), rs(n)
    dbz = 0.;  rc = 2.49e-6;  ri = 4.99e-6;  rs = 9.99e-6
    call calc_refl10cm(s(:,1), s(:,2), s(:,4), s(:,8), s(:,5), s(:,6), s(:,12), s(:,13), dbz, 1, n, 1, 1)
    call calc_effectRad(s(:,12), s(:,13), s(:,1), s(:,2), s(:,9), s(:,3), s(:,7), s(:,5), rc, ri, rs, 1, n)
    d(:,1) = dble(dbz);  d(:,2) = dble(rc);  d(:,3) = dble(ri);  d(:,4) = dble(rs)
  end subroutine diagnose

  subroutine put_table(t, shp)
    real(8), intent(in) :: t(*)
    integer, intent(in) :: shp(:)
    integer :: dims(4)
    dims = 1
    dims(1:size(shp)) = shp
    write(uout) size(shp), dims, t(1:product(shp))
  end subroutine put_table

  subroutine tables_mode()
    call put_table(tcg_racg, shape(tcg_racg));   call put_table(tmr_racg, shape(tmr_racg))
    call put_table(tcr_gacr, shape(tcr_gacr));   call put_table(tmg_gacr, shape(tmg_gacr))
    call put_table(tnr_racg, shape(tnr_racg));   call put_table(tnr_gacr, shape(tnr_gacr))
    call put_table(tcs_racs1, shape(tcs_racs1)); call put_table(tmr_racs1, shape(tmr_racs1))
    call put_table(tcs_racs2, shape(tcs_racs2)); call put_table(tmr_racs2, shape(tmr_racs2))
    call put_table(tcr_sacr1, shape(tcr_sacr1)); call put_table(tms_sacr1, shape(tms_sacr1))
    call put_table(tcr_sacr2, shape(tcr_sacr2)); call put_table(tms_sacr2, shape(tms_sacr2))
    call put_table(tnr_racs1, shape(tnr_racs1)); call put_table(tnr_racs2, shape(tnr_racs2))
    call put_table(tnr_sacr1, shape(tnr_sacr1)); call put_table(tnr_sacr2, shape(tnr_sacr2))
    call put_table(tpi_qcfz, shape(tpi_qcfz));   call put_table(tni_qcfz, shape(tni_qcfz))
    call put_table(tpi_qrfz, shape(tpi_qrfz));   call put_table(tpg_qrfz, shape(tpg_qrfz))
    call put_table(tni_qrfz, shape(tni_qrfz));   call put_table(tnr_qrfz, shape(tnr_qrfz))
    call put_table(tps_iaus, shape(tps_iaus));   call put_table(tni_iaus, shape(tni_iaus))
    call put_table(tpi_ide, shape(tpi_ide))
    call put_table(t_Efrw, shape(t_Efrw));       call put_table(t_Efsw, shape(t_Efsw))
    call put_table(tnc_wev, shape(tnc_wev))
    write(uout) dble(t1_qr_qc), dble(t1_qr_qi), dble(t2_qr_qi), dble(t1_qg_qc), dble(t1_qs_qc), dble(t1_qs_qi), &
         dble(t1_qr_ev), dble(t2_qr_ev), dble(t1_qs_sd), dble(t2_qs_sd), dble(t1_qg_sd), dble(t2_qg_sd), &
         dble(t1_qs_me), dble(t2_qs_me), dble(t1_qg_me), dble(t2_qg_me)
  end subroutine tables_mode

  subroutine adapter_mode()
    integer :: n, mx, i, k, ih, im, m
    double precision :: p064, rcp64
    real, allocatable :: f(:,:), h(:,:,:,:), z(:)
    double precision, allocatable :: oh(:,:,:,:)
    read(uin) mx, n, p064, rcp64
    nx = mx;  nz = n;  p0 = real(p064);  r_on_cp = real(rcp64)
    call alloc_columns(nz, nx)
    allocate(f(nz,nx), h(nz,nx,5,2), z(nz), oh(nz,nx,5,2))
    read(uin) f;  theta = f
    read(uin) f;  dtheta_adv = f
    read(uin) f;  dtheta_div = f
    read(uin) f;  exner = f
    read(uin) z;  dz = z
    read(uin) f;  qv = f
    read(uin) f;  dqv_adv = f
    read(uin) f;  dqv_div = f
    read(uin) h
    do im = 1, 2;  do ih = 1, 5;  do i = 1, nx;  do k = 1, nz
       hydrometeors(k,i,ih)%moments(1,im) = h(k,i,ih,im)
    end do;  end do;  end do;  end do
    read(uin) h
    do im = 1, 2;  do ih = 1, 5;  do i = 1, nx;  do k = 1, nz
       dhydrometeors_adv(k,i,ih)%moments(1,im) = h(k,i,ih,im)
    end do;  end do;  end do;  end do
    read(uin) h
    do im = 1, 2;  do ih = 1, 5;  do i = 1, nx;  do k = 1, nz
       dhydrometeors_div(k,i,ih)%moments(1,im) = h(k,i,ih,im)
    end do;  end do;  end do;  end do
    nlog = 0;  recording = .true.
    call mphys_thompson09_interfacen
    recording = .false.
    do im = 1, 2;  do ih = 1, 5;  do i = 1, nx;  do k = 1, nz
       oh(k,i,ih,im) = dble(dhydrometeors_mphys(k,i,ih)%moments(1,im))
    end do;  end do;  end do;  end do
    write(uout) dble(dtheta_mphys), dble(dqv_mphys), oh, nlog
    do m = 1, nlog
       write(uout) log_form(m), log_name(m), log_k(m), log_i(m), log_v(m)
    end do
  end subroutine adapter_mode

end program ref_driver
