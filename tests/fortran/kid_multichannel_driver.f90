! Several channels through the Fortran drop-in (kid_amd/fortran): radiometer_multi_batch and mie_radar_multi_batch of
! module_mp_thompson09n, built against the KiD stand-ins of kid_stubs.f90 with the default REAL of the build (8 bytes in
! build/, 4 bytes in build32/).
!
!   kid_multichannel_driver FILE [warm]
!       FILE = "nz ncol nch", then nch lines "wavelength eps_w_re eps_w_im eps_i_re eps_i_im kw2 mu emissivity t_cosmic", then
!       "rho_w rho_i", then nz lines "dz k_gas(1..nch)", then ncol lines "t_sfc", then ncol*nz lines "t p qv qc qr nr qs qg w",
!       column after column, kts first.  Every output of both operators is asked for; warm: an iiwarm run, and the optional
!       qc, qs, qg, w, k_gas_ch, t_sfc, rho_w, rho_i, kw2, mu, emissivity and t_cosmic are left out.
!       Prints "RAD name c i k value" and "MIE name c i k value" for every profile, with k = 0 for the numbers of a column.
program kid_multichannel_driver
  use, intrinsic :: iso_c_binding, only: c_double
  use namelists, only: iiwarm
  use module_mp_thompson09n, only: radiometer_multi_batch, mie_radar_multi_batch, thompson_finalize
  implicit none
  character(1024) :: path
  character(64) :: arg
  integer :: n, ncol, nch, c, i, k, u, v
  logical :: warm
  real(c_double) :: rho(2)
  real(c_double), allocatable :: cf(:,:)
  real, allocatable, dimension(:,:) :: t, p, qv, qc, qr, nr, qs, qg, w, k_gas
  real, allocatable :: dz(:), t_sfc(:), o(:,:,:,:), s(:,:,:), m(:,:,:,:), pt(:,:)
  character(9), parameter :: rnames(9) = (/ 'k_abs    ', 'k_bsc    ', 'refl     ', 'trans    ', 'tb_up    ', 'tb_down  ', &
       'tb_toa   ', 'tb_ground', 'tau_abs  ' /)
  character(9), parameter :: mnames(14) = (/ 'dbz      ', 'dbz_up   ', 'dbz_down ', 'dbz_r    ', 'dbz_s    ', 'dbz_g    ', &
       'mie_r    ', 'mie_s    ', 'mie_g    ', 'ext      ', 'pia_up   ', 'pia_down ', 'vd       ', 'pia_total' /)

  if (command_argument_count() < 1) then
     write(*,'(a)') ' kid_multichannel_driver: FILE [warm]'
     stop 2
  end if
  call get_command_argument(1, path)
  arg = 'full'
  if (command_argument_count() >= 2) call get_command_argument(2, arg)
  warm = trim(arg) == 'warm'
  open(newunit=u, file=trim(path), status='old', action='read')
  read(u, *) n, ncol, nch
  allocate(cf(9,nch))
  do c = 1, nch
     read(u, *) cf(:,c)
  end do
  read(u, *) rho
  allocate(dz(n), k_gas(n,nch), t_sfc(ncol))
  do k = 1, n
     read(u, *) dz(k), k_gas(k,:)
  end do
  do i = 1, ncol
     read(u, *) t_sfc(i)
  end do
  allocate(t(n,ncol), p(n,ncol), qv(n,ncol), qc(n,ncol), qr(n,ncol), nr(n,ncol), qs(n,ncol), qg(n,ncol), w(n,ncol))
  allocate(o(n,ncol,nch,6), s(ncol,nch,3), m(n,ncol,nch,13), pt(ncol,nch))
  do i = 1, ncol
     do k = 1, n
        read(u, *) t(k,i), p(k,i), qv(k,i), qc(k,i), qr(k,i), nr(k,i), qs(k,i), qg(k,i), w(k,i)
     end do
  end do
  close(u)
  iiwarm = warm
  if (warm) then
     call radiometer_multi_batch(nch, ncol, n, cf(1,:), cf(2,:), cf(3,:), cf(4,:), cf(5,:), t, p, qv, qr, nr, o(:,:,:,1), &
          o(:,:,:,2), o(:,:,:,3), o(:,:,:,4), o(:,:,:,5), o(:,:,:,6), s(:,:,1), s(:,:,2), s(:,:,3), dz=dz)
     call mie_radar_multi_batch(nch, ncol, n, cf(1,:), cf(2,:), cf(3,:), cf(4,:), cf(5,:), t, p, qv, qr, nr, m(:,:,:,1), &
          m(:,:,:,2), m(:,:,:,3), m(:,:,:,4), m(:,:,:,5), m(:,:,:,6), m(:,:,:,7), m(:,:,:,8), m(:,:,:,9), m(:,:,:,10), &
          m(:,:,:,11), m(:,:,:,12), m(:,:,:,13), pt, dz=dz)
  else
     call radiometer_multi_batch(nch, ncol, n, cf(1,:), cf(2,:), cf(3,:), cf(4,:), cf(5,:), t, p, qv, qr, nr, o(:,:,:,1), &
          o(:,:,:,2), o(:,:,:,3), o(:,:,:,4), o(:,:,:,5), o(:,:,:,6), s(:,:,1), s(:,:,2), s(:,:,3), qc=qc, qs=qs, qg=qg, dz=dz, &
          k_gas_ch=k_gas, t_sfc=t_sfc, rho_w=rho(1), rho_i=rho(2), mu=cf(7,:), emissivity=cf(8,:), t_cosmic=cf(9,:))
     call mie_radar_multi_batch(nch, ncol, n, cf(1,:), cf(2,:), cf(3,:), cf(4,:), cf(5,:), t, p, qv, qr, nr, m(:,:,:,1), &
          m(:,:,:,2), m(:,:,:,3), m(:,:,:,4), m(:,:,:,5), m(:,:,:,6), m(:,:,:,7), m(:,:,:,8), m(:,:,:,9), m(:,:,:,10), &
          m(:,:,:,11), m(:,:,:,12), m(:,:,:,13), pt, qc=qc, qs=qs, qg=qg, dz=dz, w=w, k_gas_ch=k_gas, rho_w=rho(1), &
          rho_i=rho(2), kw2=cf(6,:))
  end if
  do v = 1, 6
     do c = 1, nch
        do i = 1, ncol
           do k = 1, n
              write(*, '(a,1x,a,3i6,es26.17e3)') 'RAD', trim(rnames(v)), c, i, k, o(k,i,c,v)
           end do
        end do
     end do
  end do
  do v = 1, 3
     do c = 1, nch
        do i = 1, ncol
           write(*, '(a,1x,a,3i6,es26.17e3)') 'RAD', trim(rnames(6 + v)), c, i, 0, s(i,c,v)
        end do
     end do
  end do
  do v = 1, 13
     do c = 1, nch
        do i = 1, ncol
           do k = 1, n
              write(*, '(a,1x,a,3i6,es26.17e3)') 'MIE', trim(mnames(v)), c, i, k, m(k,i,c,v)
           end do
        end do
     end do
  end do
  do c = 1, nch
     do i = 1, ncol
        write(*, '(a,1x,a,3i6,es26.17e3)') 'MIE', trim(mnames(14)), c, i, 0, pt(i,c)
     end do
  end do
  call thompson_finalize
end program kid_multichannel_driver
