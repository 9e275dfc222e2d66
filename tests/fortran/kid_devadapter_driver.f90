! The adapter's l_device_adapter through the Fortran boundary: the KiD time loop of kid_mini_driver with the switch that
! moves the gather (W:59-97) and the back-out (W:198-245) into the library call.
!
!   kid_devadapter_driver nx nsteps case [key=value ...]
!     case        warm | mixed: the columns of kid_mini_driver (KAT-B / KAT-A of SURVEY 9h)
!     adapter=1   mphys_thompson09n's l_device_adapter = .true. (default 0: the host loops)
!     arith=p32n  module_mp_thompson09n's kidmp_arith (p64 default; p32n / f32 need 4-byte default REAL)
!     forcing=1   the prescribed updraft + divergence forcing of kid_mini_driver
!     mphys=<n>   write inputs, forcing terms and the d*_mphys outputs of step n to mphys_dump.txt (kid_mini_driver's format)
!     dump=<n>    write every save_dg call made during step n to dg_dump.txt
!     radar=1, radii=1   l_radar_reflectivity, l_effective_radii
!     rates=0     l_rate_diagnostics = .false.
!     devices=a,b kidmp_ndevices / kidmp_devices
!     time=1      time the step loop: "TIME <steps> <seconds> <column-steps/s>" (the state is then not advanced)
! Prints the end-state sums of column 1 ("KATB") and of column nx ("KATBN").
program kid_devadapter_driver
  use parameters, only: nz, nx, dt
  use column_variables
  use namelists, only: iiwarm, set_Nc
  use diagnostics, only: recording, nlog, dump_log
  use mphys_thompson09n, only: mphys_thompson09_interfacen, l_device_adapter, l_radar_reflectivity, l_effective_radii
  use module_mp_thompson09n, only: thompson_finalize, kidmp_arith, l_rate_diagnostics, kidmp_ndevices, kidmp_devices
  implicit none
  integer :: k, i, n, j, nsteps, dump_step, mphys_step, a, eq, up, dn
  integer(8) :: c0, c1, crate
  real :: z, p, t, es, qsat, w
  logical :: forcing, timing
  character(64) :: arg, which, key, val

  nsteps = 360; which = 'warm'; dump_step = 0; mphys_step = 0; forcing = .false.; timing = .false.
  if (command_argument_count() < 3) then
     write(*,'(a)') ' usage: kid_devadapter_driver nx nsteps warm|mixed [key=value ...]'
     stop 2
  end if
  call get_command_argument(1, arg); read(arg,*) nx
  call get_command_argument(2, arg); read(arg,*) nsteps
  call get_command_argument(3, which)
  do a = 4, command_argument_count()
     call get_command_argument(a, arg)
     eq = index(arg, '=')
     if (eq == 0) then
        write(*,'(2a)') ' kid_devadapter_driver: expected key=value, got ', trim(arg)
        stop 2
     end if
     key = arg(1:eq-1);  val = arg(eq+1:)
     select case (trim(key))
     case ('adapter');  l_device_adapter = trim(val) == '1'
     case ('arith');    kidmp_arith = val(1:4)
     case ('forcing');  forcing = trim(val) == '1'
     case ('mphys');    read(val,*) mphys_step
     case ('dump');     read(val,*) dump_step
     case ('radar');    l_radar_reflectivity = trim(val) == '1'
     case ('radii');    l_effective_radii = trim(val) == '1'
     case ('rates');    l_rate_diagnostics = trim(val) /= '0'
     case ('time');     timing = trim(val) == '1'
     case ('devices')
        kidmp_ndevices = 2
        read(val,*) kidmp_devices(1), kidmp_devices(2)
     case default
        write(*,'(2a)') ' kid_devadapter_driver: unknown option ', trim(arg)
        stop 2
     end select
  end do
  iiwarm = trim(which) /= 'mixed'; set_Nc = 100.0
  call alloc_columns(nz, nx)
  do i = 1, nx
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
  if (forcing) then                            ! the updraft w(z) = 2 sin(pi z / ztop) m/s and the 2e-5 /s sink of kid_mini_driver
     do i = 1, nx
        do k = 1, nz
           z = (k-0.5)*dz(k)
           w = 2.0*sin(3.14159265*z/(nz*dz(k)))*(1. + 0.05*(i-1))
           up = min(k+1, nz);  dn = max(k-1, 1)
           dtheta_adv(k,i) = -w*(theta(up,i) - theta(dn,i))/((up-dn)*dz(k))
           dqv_adv(k,i)    = -w*(qv(up,i) - qv(dn,i))/((up-dn)*dz(k))
           dtheta_div(k,i) = -2.e-5*(theta(k,i) - theta(1,i))
           dqv_div(k,i)    = -2.e-5*qv(k,i)
           do j = 1, 5
              dhydrometeors_adv(k,i,j)%moments = -w*(hydrometeors(up,i,j)%moments - hydrometeors(dn,i,j)%moments) &
                   /((up-dn)*dz(k))
              dhydrometeors_div(k,i,j)%moments = -2.e-5*hydrometeors(k,i,j)%moments
           end do
        end do
     end do
  end if
  if (timing) then                             ! initialisation (tables, staging memory, first touch) is not the step loop
     call mphys_thompson09_interfacen
     call system_clock(c0, crate)
  end if
  do n = 1, nsteps
     recording = n == dump_step
     if (recording) nlog = 0
     call mphys_thompson09_interfacen
     if (recording) call dump_log('dg_dump.txt')
     if (n == mphys_step) then
        open(23, file='mphys_dump.txt', status='replace')
        do i = 1, nx
           do k = 1, nz
              write(23,'(38es25.17)') theta(k,i), exner(k,i), qv(k,i), dz(k), &
                   hydrometeors(k,i,1)%moments(1,1), hydrometeors(k,i,2)%moments(1,1), hydrometeors(k,i,2)%moments(1,2), &
                   hydrometeors(k,i,3)%moments(1,1), hydrometeors(k,i,3)%moments(1,2), hydrometeors(k,i,4)%moments(1,1), &
                   hydrometeors(k,i,5)%moments(1,1), &
                   dtheta_adv(k,i), dtheta_div(k,i), dqv_adv(k,i), dqv_div(k,i), &
                   dhydrometeors_adv(k,i,1)%moments(1,1), dhydrometeors_adv(k,i,2)%moments(1,1), dhydrometeors_adv(k,i,2)%moments(1,2), &
                   dhydrometeors_adv(k,i,3)%moments(1,1), dhydrometeors_adv(k,i,3)%moments(1,2), dhydrometeors_adv(k,i,4)%moments(1,1), &
                   dhydrometeors_adv(k,i,5)%moments(1,1), &
                   dhydrometeors_div(k,i,1)%moments(1,1), dhydrometeors_div(k,i,2)%moments(1,1), dhydrometeors_div(k,i,2)%moments(1,2), &
                   dhydrometeors_div(k,i,3)%moments(1,1), dhydrometeors_div(k,i,3)%moments(1,2), dhydrometeors_div(k,i,4)%moments(1,1), &
                   dhydrometeors_div(k,i,5)%moments(1,1), &
                   dtheta_mphys(k,i), dqv_mphys(k,i), &
                   dhydrometeors_mphys(k,i,1)%moments(1,1), dhydrometeors_mphys(k,i,2)%moments(1,1), dhydrometeors_mphys(k,i,2)%moments(1,2), &
                   dhydrometeors_mphys(k,i,3)%moments(1,1), dhydrometeors_mphys(k,i,3)%moments(1,2), dhydrometeors_mphys(k,i,4)%moments(1,1), &
                   dhydrometeors_mphys(k,i,5)%moments(1,1)
           end do
        end do
        close(23)
     end if
     if (timing) cycle
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
  if (timing) then
     call system_clock(c1)
     write(*,'(a,i0,1x,es14.6,1x,es14.6)') 'TIME ', nsteps, real(c1-c0,8)/real(crate,8), &
          real(nx,8)*real(nsteps,8)*real(crate,8)/real(max(c1-c0,1_8),8)
  end if
  write(*,'(a,4es24.16)') 'KATB ', sum(qv(:,1)), sum(hydrometeors(:,1,1)%moments(1,1)), &
       sum(hydrometeors(:,1,2)%moments(1,1)), sum(hydrometeors(:,1,2)%moments(1,2))
  write(*,'(a,4es24.16)') 'KATBN', sum(qv(:,nx)), sum(hydrometeors(:,nx,1)%moments(1,1)), &
       sum(hydrometeors(:,nx,2)%moments(1,1)), sum(hydrometeors(:,nx,2)%moments(1,2))
  call thompson_finalize
end program kid_devadapter_driver
