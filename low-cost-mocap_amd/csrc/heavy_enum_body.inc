// heavy_enum_body.inc -- the body of the heavy-root enumeration kernels (csrc/heavy_bb.hip includes it once per __global__:
// the identical-K kernel and the per-camera-K one are the same text; HV_PERK says which).  In scope: HeavyArgs a, F32R.
  constexpr bool PERK = HV_PERK;
  __shared__ uint16_t s_n[kMaxCameras];
  __shared__ uint8_t s_lvl[kMaxCameras];
  __shared__ uint8_t s_dcam[kMaxCameras];
  __shared__ uint8_t s_pos[PERK ? kMaxCameras : 1];  // PERK: position of a camera among the root's seen cameras = its intrinsics index
  __shared__ int s_m, s_slice, s_last;
  __shared__ uint32_t s_G;
  __shared__ unsigned long long s_best, s_gbest;
  __shared__ uint8_t s_dg[kHvGlobalEnumDigits][kHvEnumThreads];
  // the root's hits, tabulated once: DLT contribution (dlt_contribution: the function every path of the core rounds with) and
  // pixel coordinates of hit d of camera c at entry s_off[c] + d
  __shared__ double s_tab[kHvEnumTab][10];
  __shared__ float2 s_xy[kHvEnumTab];
  __shared__ uint16_t s_off[kMaxCameras + 1];
  __shared__ int s_split, s_csplit, s_views;
  __shared__ uint32_t s_Npre, s_Psuf;
  const int tid = threadIdx.x;
  const int C = a.cv.C, M = a.M;
  int n_roots = *a.enum_count;
  if (n_roots > a.enum_max) n_roots = a.enum_max;
  const double inf = __builtin_huge_val();
  for (int s = 0; s < n_roots; s++) {
    const int h = a.enum_list[s];
    const unsigned char* rec = a.recs + (size_t)h * a.stride;
    const HeavyRecHdr hd = *reinterpret_cast<const HeavyRecHdr*>(rec);
    const uint16_t* nc = reinterpret_cast<const uint16_t*>(rec + heavy_rec_counts_off());
    const uint8_t* hl = rec + heavy_rec_hits_off(C);
    const int Hs = hd.Hs;
    const float2* fb = (const float2*)(a.blobs + (size_t)hd.frame * C * M * 2);
    const size_t o = (size_t)hd.frame * a.K_big + hd.outslot;
    block_sync_lds();  // (the previous root's shared state is dead)
    if (tid < C) s_n[tid] = nc[tid];
    if (tid == 0) {
      int m = 0;
      unsigned long long G = 1;
      for (int c = 0; c < C; c++) {
        s_lvl[c] = 0xFF;
        if (nc[c] > 1) {
          s_lvl[c] = (uint8_t)m;
          s_dcam[m++] = (uint8_t)c;
          G *= nc[c];
        }
      }
      s_m = m;
      s_G = (uint32_t)G;  // (<= 2^24: heavy_bb_kernel queued it)
      s_best = 0x7ff0000000000000ull;
      s_gbest = ~0ull;
      int off = 0, views = 0;
      for (int c = 0; c < C; c++) {
        s_off[c] = (uint16_t)(off < 0xFFFF ? off : 0xFFFF);
        if constexpr (PERK) s_pos[c] = (uint8_t)views;
        off += nc[c];
        views += nc[c] ? 1 : 0;
      }
      s_off[C] = (uint16_t)(off < 0xFFFF ? off : 0xFFFF);
      s_views = views;
      // The digits split into a PREFIX (the multi-hit cameras with the lowest camera numbers = the fastest digits of the
      // candidate index) and a SUFFIX (the last ones, >= 64 combinations where the root has them).  A lane takes one prefix
      // and walks the suffix combinations: B is summed in camera order from zeros (mocap_device.hpp triangulate_and_score), so
      // the partial sum over the cameras before the first suffix camera is the same for all of them -- computed once, the very
      // bits the full left-to-right sum passes through.
      int split = m;
      uint32_t psuf = 1;
      while (split > 0 && psuf < 64u) psuf *= nc[s_dcam[--split]];
      s_split = split;
      s_Psuf = psuf;
      s_Npre = (uint32_t)(G / psuf);
      s_csplit = split < m ? s_dcam[split] : C;
    }
    __syncthreads();
    const int m = s_m;
    const uint32_t G = s_G;
    const bool tabbed = s_off[C] <= kHvEnumTab;  // (uniform) else: every group from its raw observations, as before
    if (tabbed) {
      for (int c = 0; c < C; c++) {
        const int n = s_n[c];
        // (PERK: the loop's camera is the same for the whole workgroup, so is its position: the table reads stay scalar loads)
        const size_t pq_c = PERK ? 12 * ((size_t)__builtin_amdgcn_readfirstlane((int)s_pos[c]) * C + c) : (size_t)12 * c;
        if (tid < n) {
          const float2 w = fb[(size_t)c * M + hl[(size_t)c * Hs + tid]];
          double Bc[10];
          dlt_contribution(Bc, a.cv.pq(pq_c), (double)w.x, (double)w.y);
#pragma unroll
          for (int e = 0; e < 10; e++) s_tab[s_off[c] + tid][e] = Bc[e];
          s_xy[s_off[c] + tid] = w;
        }
      }
      __syncthreads();
    }
    const int split = s_split, csplit = s_csplit, views = s_views;
    const uint32_t Npre = s_Npre, Psuf = s_Psuf;
    const uint32_t n_slices = tabbed ? (Npre + kHvEnumThreads - 1) / kHvEnumThreads : (G + kHvEnumSlice - 1) / kHvEnumSlice;
    EigCut ec;
    {
      const double om = (double)__int_as_float(hd.omax_bits);
      ec.p3max2 = a.p3max2;
      ec.o2slack = (1100.0 * 0x1p-46) * (om * om);
    }
    double be = inf, bX[3] = {0, 0, 0};
    uint32_t bg = 0;
    while (true) {
      if (tid == 0) s_slice = atomicAdd(&a.enum_slice[s], 1);
      __syncthreads();
      const uint32_t sl = (uint32_t)s_slice;
      __syncthreads();
      if (sl >= n_slices) break;  // (uniform)
      if (tabbed) {
        const uint32_t q = sl * (uint32_t)kHvEnumThreads + (uint32_t)tid;  // this lane's prefix
        if (q < Npre) {
          uint32_t rem = q;
          for (int j = 0; j < split; j++) {
            uint32_t qd, d;
            divmod_small(rem, (uint32_t)s_n[s_dcam[j]], qd, d);
            rem = qd;
            s_dg[j][tid] = (uint8_t)d;
          }
          double Bp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          for (int c = 0; c < csplit; c++) {
            const int n = s_n[c];
            if (n) {
              const double* t = s_tab[s_off[c] + (n > 1 ? (int)s_dg[s_lvl[c]][tid] : 0)];
#pragma unroll
              for (int e = 0; e < 10; e++) Bp[e] = Bp[e] + t[e];
            }
          }
          auto obs = [&](int c, double& x, double& y) -> bool {
            const int n = s_n[c];
            if (!n) return false;
            const float2 w = s_xy[s_off[c] + (n > 1 ? (int)s_dg[s_lvl[c]][tid] : 0)];
            x = (double)w.x;
            y = (double)w.y;
            return true;
          };
          for (uint32_t sfx = 0; sfx < Psuf; sfx++) {  // ascending candidate index: g = q + Npre * sfx
            uint32_t r2 = sfx;
            for (int j = split; j < m; j++) {
              uint32_t qd, d;
              divmod_small(r2, (uint32_t)s_n[s_dcam[j]], qd, d);
              r2 = qd;
              s_dg[j][tid] = (uint8_t)d;
            }
            double B[10];
#pragma unroll
            for (int e = 0; e < 10; e++) B[e] = Bp[e];
            for (int c = csplit; c < C; c++) {
              const int n = s_n[c];
              if (n) {
                const double* t = s_tab[s_off[c] + (n > 1 ? (int)s_dg[s_lvl[c]][tid] : 0)];
#pragma unroll
                for (int e = 0; e < 10; e++) B[e] = B[e] + t[e];
              }
            }
            double X[3], e = inf;
            const double bound = __longlong_as_double((long long)__hip_atomic_load(&a.enum_bound[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            // (the call triangulate_and_score ends in, with the B it would have summed)
            solve_and_score<!PERK, true, F32R, false, 1>(a.cv, B, views, obs, X, e, bound * (double)(2 * views) * (1.0 + 0x1p-40), ec);
            if (e < be) {  // strict <: the first minimum of this lane's ascending run
              be = e;
              bg = q + Npre * sfx;
              bX[0] = X[0]; bX[1] = X[1]; bX[2] = X[2];
              atomicMin(&a.enum_bound[s], (unsigned long long)__double_as_longlong(e));
            }
          }
        }
        continue;
      }
      const uint32_t g1 = (sl + 1) * (uint32_t)kHvEnumSlice < G ? (sl + 1) * (uint32_t)kHvEnumSlice : G;
      for (uint32_t g = sl * (uint32_t)kHvEnumSlice + (uint32_t)tid; g < g1; g += kHvEnumThreads) {
        // digits of g: the first multi-hit camera is the fastest one (helpers.py:394-400 order, as in frame_kernel.hip)
        uint32_t rem = g;
        for (int j = 0; j < m; j++) {
          uint32_t qd, d;
          divmod_small(rem, (uint32_t)s_n[s_dcam[j]], qd, d);
          rem = qd;
          s_dg[j][tid] = (uint8_t)d;
        }
        auto obs = [&](int c, double& x, double& y) -> bool {
          const int n = s_n[c];
          if (!n) return false;
          const int d = n > 1 ? s_dg[s_lvl[c]][tid] : 0;
          const float2 w = fb[(size_t)c * M + hl[(size_t)c * Hs + d]];
          x = (double)w.x;
          y = (double)w.y;
          return true;
        };
        double X[3], e = inf;
        const double bound = __longlong_as_double((long long)__hip_atomic_load(&a.enum_bound[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        triangulate_and_score<!PERK, true, F32R, 1, false>(a.cv, obs, obs, X, e, bound, ec);
        if (e < be) {  // strict <: the first minimum of this lane's ascending run
          be = e;
          bg = g;
          bX[0] = X[0]; bX[1] = X[1]; bX[2] = X[2];
          atomicMin(&a.enum_bound[s], (unsigned long long)__double_as_longlong(e));
        }
      }
    }
    // the workgroup's winner: smallest error bits, then smallest group index among its holders
    if (be < inf) atomicMin(&s_best, (unsigned long long)__double_as_longlong(be));
    __syncthreads();
    const unsigned long long wb = s_best;
    if (be < inf && (unsigned long long)__double_as_longlong(be) == wb) atomicMin(&s_gbest, (unsigned long long)bg);
    __syncthreads();
    HvPart* part = reinterpret_cast<HvPart*>(a.enum_part) + (size_t)s * a.enum_grid;
    if (wb == 0x7ff0000000000000ull) {
      if (tid == 0) {
        q_st(&part[blockIdx.x].ebits, wb);  // (agent-scope stores: the merging workgroup may sit on another XCD)
        q_st(&part[blockIdx.x].g, 0xFFFFFFFFu);
      }
    } else if (be < inf && (unsigned long long)__double_as_longlong(be) == wb && (unsigned long long)bg == s_gbest) {  // (one lane)
      q_st(&part[blockIdx.x].ebits, wb);
      q_st(&part[blockIdx.x].g, bg);
      q_st(&part[blockIdx.x].X[0], bX[0]);
      q_st(&part[blockIdx.x].X[1], bX[1]);
      q_st(&part[blockIdx.x].X[2], bX[2]);
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(&a.enum_done[s], 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) continue;  // (uniform)
    // ---- the last workgroup to report merges (its loads see the others' records: each was fenced before its count)
    __threadfence();
    if (tid == 0) {
      s_best = 0x7ff0000000000000ull;
      s_gbest = ~0ull;
    }
    __syncthreads();
    for (int w = tid; w < (int)gridDim.x; w += kHvEnumThreads) {
      const unsigned long long eb = __hip_atomic_load(&part[w].ebits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (eb != 0x7ff0000000000000ull) atomicMin(&s_best, eb);
    }
    __syncthreads();
    const unsigned long long fb_ = s_best;
    if (fb_ == 0x7ff0000000000000ull) continue;  // no group with a finite error: the frame kernel's group 0 stands
    for (int w = tid; w < (int)gridDim.x; w += kHvEnumThreads)
      if (__hip_atomic_load(&part[w].ebits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == fb_)
        atomicMin(&s_gbest, (unsigned long long)__hip_atomic_load(&part[w].g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();
    const uint32_t gw = (uint32_t)s_gbest;
    for (int w = tid; w < (int)gridDim.x; w += kHvEnumThreads) {
      if (__hip_atomic_load(&part[w].ebits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == fb_ &&
          __hip_atomic_load(&part[w].g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gw) {  // (one record: a group lives in one slice)
        const double X[3] = {__hip_atomic_load(&part[w].X[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                             __hip_atomic_load(&part[w].X[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                             __hip_atomic_load(&part[w].X[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
        FrameArgs fa;  // (store_point only looks at xyz and world)
        fa.xyz = a.xyz;
        fa.world = a.world;
        store_point(fa, o, X);
        a.err[o] = __longlong_as_double((long long)fb_);
        uint32_t rem = gw;
        uint8_t dg[kHvGlobalEnumDigits];
        for (int j = 0; j < m; j++) {
          uint32_t qd, d;
          divmod_small(rem, (uint32_t)s_n[s_dcam[j]], qd, d);
          rem = qd;
          dg[j] = (uint8_t)d;
        }
        for (int c = 0; c < C; c++) {
          const int n = s_n[c];
          int16_t sidx = -1;
          if (n) {
            int d = 0;
            if (n > 1)
              for (int j = 0; j < m; j++)
                if (s_dcam[j] == c) d = dg[j];
            sidx = (int16_t)hl[(size_t)c * Hs + d];
          }
          a.corr[o * C + c] = sidx;
        }
      }
    }
  }
