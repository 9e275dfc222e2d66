! A droplet number per column through the Fortran boundary: the KiD 1-D warm-rain case (KAT-B of SURVEY 9h, as
! kid_mini_driver's `warm`) replicated over nx columns, x being the axis of an Nd ensemble -- the adapter's
! set_Nc_column cycles over a short list, all members advance in one launch per step.
!
!   kid_ncol_driver [nx [nsteps [dump_step [nc=a,b,c [ncsize=n]]]]]
!     nx         columns (default 3)
!     nsteps     time steps (default 60)
!     dump_step  write every save_dg call made during that step to dg_dump.txt (0: none), as kid_mini_driver does
!     nc=a,b,c   set_Nc_column(i) = the (mod(i-1, n) + 1)-th value of the list, cm**-3; without it set_Nc_column stays
!                unallocated and the run is kid_mini_driver's, call for call
!     ncsize=n   allocate set_Nc_column(n) instead of (nx): any n but nx is a misuse the adapter stops on
! Prints kid_mini_driver's KATB / KATBN lines and writes the end state of every column and level to
! ncol_end_state.txt: theta, qv, qc, qr, nr.
program kid_ncol_driver
  use parameters, only: nz, nx, dt
  use column_variables
  use namelists, only: iiwarm, set_Nc
  use diagnostics, only: recording, nlog, dump_log
  use mphys_thompson09n, only: mphys_thompson09_interfacen, set_Nc_column
  use module_mp_thompson09n, only: thompson_finalize
  implicit none
  integer :: k, i, n, j, nsteps, dump_step, a, nv, pos, nxt, ios, ncsize
  real :: z, p, t, vals(16)
  character(256) :: arg

  nx = 3; nsteps = 60; dump_step = 0; nv = 0; ncsize = -1
  if (command_argument_count() >= 1) then
     call get_command_argument(1, arg); read(arg,*) nx
  end if
  if (command_argument_count() >= 2) then
     call get_command_argument(2, arg); read(arg,*) nsteps
  end if
  if (command_argument_count() >= 3) then
     call get_command_argument(3, arg); read(arg,*) dump_step
  end if
  do a = 4, command_argument_count()
     call get_command_argument(a, arg)
     if (arg(1:7) == 'ncsize=') then
        read(arg(8:), *) ncsize
        cycle
     end if
     if (arg(1:3) /= 'nc=') then
        write(*,'(2a)') ' kid_ncol_driver: unknown option ', trim(arg)
        stop 2
     end if
     pos = 4
     do while (pos <= len_trim(arg) .and. nv < 16)
        nxt = index(arg(pos:), ',')
        if (nxt == 0) nxt = len_trim(arg) - pos + 2
        nv = nv + 1
        read(arg(pos:pos+nxt-2), *, iostat=ios) vals(nv)
        if (ios /= 0) then
           write(*,'(2a)') ' kid_ncol_driver: cannot read ', trim(arg)
           stop 2
        end if
        pos = pos + nxt
     end do
  end do
  iiwarm = .true.; set_Nc = 100.0
  call alloc_columns(nz, nx)
  do i = 1, nx
     do k = 1, nz
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
     end do
  end do
  if (nv > 0) then
     if (ncsize < 0) ncsize = nx
     allocate(set_Nc_column(ncsize))
     do i = 1, ncsize
        set_Nc_column(i) = vals(mod(i-1, nv) + 1)
     end do
  end if
  do n = 1, nsteps
     recording = n == dump_step
     if (recording) nlog = 0
     call mphys_thompson09_interfacen
     if (recording) call dump_log('dg_dump.txt')
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
  open(24, file='ncol_end_state.txt', status='replace')
  do i = 1, nx
     do k = 1, nz
        write(24,'(5es25.17)') theta(k,i), qv(k,i), hydrometeors(k,i,1)%moments(1,1), &
             hydrometeors(k,i,2)%moments(1,1), hydrometeors(k,i,2)%moments(1,2)
     end do
  end do
  close(24)
  write(*,'(a,4es24.16)') 'KATB ', sum(qv(:,1)), sum(hydrometeors(:,1,1)%moments(1,1)), &
       sum(hydrometeors(:,1,2)%moments(1,1)), sum(hydrometeors(:,1,2)%moments(1,2))
  write(*,'(a,4es24.16)') 'KATBN', sum(qv(:,nx)), sum(hydrometeors(:,nx,1)%moments(1,1)), &
       sum(hydrometeors(:,nx,2)%moments(1,1)), sum(hydrometeors(:,nx,2)%moments(1,2))
  call thompson_finalize
end program kid_ncol_driver
