// vw_pair_rows.inc -- the body of the round-trip kernels (vw_pair.hip), included once per kernel template: T, L, FMA
// and KEEP (the number of detail planes below d_J kept in registers) are the including kernel's, q its PairArgs<T>.
// Text rather than a __device__ function: a kernel's own body is where the compiler folds the launch's workgroup
// size into kernel-argument reads, and KEEP = 0 must stay the kernel it was, instruction for instruction.
  constexpr int V = VT<T>::V;
  constexpr int NV = 4;
  const FwdArgs<T>& p = q.f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = p.N;
  const int nvec = N / V;
  const long long G = gridDim.x;
  const size_t plane = (size_t)p.B * (size_t)(unsigned)p.N;
  const unsigned slab = blockDim.x * 16u;  // bytes between a lane's vectors
  long long b = blockIdx.x;
  if (b >= p.B) return;
  int cur = 0;
  dma_row<T>(reinterpret_cast<T*>(smem) + p.hlpad, p.x + b * p.ldx, nvec, p.dma_nt != 0);
  wait_vmem();
  for (;;) {
    const FwdArgs<T>& p0 = *reread(&q.f);  // the row's share of the arguments, read here (as every level's below)
    T* X = reinterpret_cast<T*>(smem) + (cur ? p0.region1 : 0) + p0.hlpad;
    T* Y = reinterpret_cast<T*>(smem) + (cur ? 0 : p0.region1) + p0.hlpad;
    lds_barrier();  // the row is in X (every wave's share); every read of the previous row done
    fill_halo(X, p0.N, p0.lv[0].hl, p0.lv[0].hr, p0.lv[0].mode, p0.npow2, (const T*)nullptr, 0);
    const long long bn = b + G;
    const size_t row = (size_t)b * (size_t)(unsigned)N;
    const int J = p0.J;
    T acc[NV][V];   // forward: the running approximation; inverse: a_J, then the sums
    T dlast[NV][V];  // d_J, kept from level J of the forward.  Every level writes it and the last one stays: handing
                     // fwd_level `j == J ? dlast : nullptr` makes the array's address a run-time value, and the
                     // compiler then keeps it in scratch (80 bytes per lane) instead of 16 VGPRs
    T dreg[NV][V];   // the prefetched d_{j-1}: never written but by its loads, so that no wait the compiler derives
                     // for those registers lands in the forward half or ahead of d_J's use, behind the stores in flight
    T dk[KEEP > 0 ? KEEP : 1][NV][V];  // after level J: dk[q] = d_{J-1-q}, q < KEEP (see the header)
    // ---- forward half (k_forward_persist) ----
    for (int j = 1; j <= J; ++j) {
      const FwdArgs<T>& pj = *reread(&q.f);  // this level's share of the arguments, read here
      const LevelDesc lv = pj.lv[j - 1];
      lds_barrier();  // X = level input + halo; every read of Y (previous level) done
      if (j == pj.J && bn < pj.B) dma_row<T>(Y, pj.x + bn * pj.ldx, nvec, pj.dma_nt != 0);  // next row -> free buffer
      T* dout = pj.details + (size_t)(j - 1) * plane + row;
      T* aout = (j == pj.J) ? pj.approx + row : nullptr;
      if constexpr (KEEP > 1) copy_regs<T, NV>(dk[1], dk[0]);
      if constexpr (KEEP > 0) copy_regs<T, NV>(dk[0], dlast);  // the previous level's details (none yet at j = 1)
      fwd_level<T, L, FMA, NV, false, false, true, L, VW_PAIR_STORE_AUX>(p, X, nvec, lv, dout, aout, true, 0ull, acc,
                                                                         nullptr, dlast);
      if (j < pj.J) {
        regs_to_level<T, L, NV, true>(Y, acc, nvec, pj.N, pj.lv[j], pj.npow2, (const T*)nullptr);
        T* t = X; X = Y; Y = t;
      }
    }
    // ---- inverse half (inverse_seq_plain); X: level J's input, Y: receiving the next row ----
    const PairArgs<T>& qi = *reread(&q);
    T* const R = X - qi.f.hlpad;
    lds_barrier();  // every level-J read of X done
    plain_to_level<T, NV>(R, acc, slab, qi.f.N, qi.hr[qi.f.J - 1], qi.own[qi.f.J - 1]);
    for (int j = J; j >= 1; --j) {
      const PairArgs<T>& qj = *reread(&q);
      const int s = qj.f.lv[j - 1].s;
      lds_barrier();  // R = a_j + halo
      zero_regs<T, NV>(acc);
      plain_row<T, L, FMA, NV, 4>(R, slab, s, qj.ilo, acc);
      lds_barrier();  // every approximation-branch read done
      // levels above this one, J - j: d_j is dlast (0), dk[J - j - 1] (1 .. KEEP) or reloaded
      if (j + KEEP < qj.f.J) {
        wait_vmem();  // the d_j prefetch
        plain_to_level<T, NV>(R, dreg, slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]);
      } else {  // d_j never left the registers
        bool shifted = false;
        if constexpr (KEEP > 0) {
          if (j + 1 == qj.f.J) { shifted = true; plain_to_level<T, NV>(R, dk[0], slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]); }
        }
        if constexpr (KEEP > 1) {
          if (j + 2 == qj.f.J) { shifted = true; plain_to_level<T, NV>(R, dk[1], slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]); }
        }
        if (!shifted) plain_to_level<T, NV>(R, dlast, slab, qj.f.N, qj.hr[j - 1], qj.own[j - 1]);
      }
      if (j > 1 && (KEEP == 0 || j + KEEP <= qj.f.J)) {  // the d_{j-1} prefetch (not a kept plane), in flight across the detail branch
        if (j + KEEP == qj.f.J) {  // the first one: behind this lane's own stores of d_1 .. d_{J-1} (see OWNERSHIP above)
          if (bn < qj.f.B) wait_vmcnt<3 * NV>();
          else wait_vmcnt<2 * NV>();
        }
        plain_load_row<T, NV>(dreg, qj.f.details + (size_t)(j - 2) * plane + row, slab);
      }
      lds_barrier();  // R = d_j + halo
      plain_row<T, L, FMA, NV, 4>(R, slab, s, reread(q.ihi), acc);
      if (j > 1) {
        lds_barrier();  // every detail-branch read done
        plain_to_level<T, NV>(R, acc, slab, qj.f.N, qj.hr[j - 2], qj.own[j - 2]);
      }
    }
    plain_store_row<T, NV>(q.y + row, acc, slab);
    if (bn >= p.B) break;
    // this wave's DMA share landed: J >= KEEP + 2 waited vmcnt(0) behind it; at J <= KEEP + 1 (no reload) the
    // 2 * NV coefficient stores of level J and the NV stores of y follow it
    wait_vmcnt<3 * NV>();
    cur = (cur + J) & 1;  // the buffer that was free during level J
    b = bn;
  }
