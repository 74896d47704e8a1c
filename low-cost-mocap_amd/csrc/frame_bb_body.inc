// frame_bb_body.inc -- the body of the search kernels (csrc/frame_bb.hip includes it once per __global__: the identical-K
// kernel and the per-camera-K one are the same text on two BBState types; a shared __device__ function in its place moved
// the identical-K kernels' register allocation).  In scope: FrameArgs p, smem, BB_STATE = the BBState type.
  // The re-submit's second pass behind a batch that flagged nothing (FrameArgs::n_frames_dev): the count was final before this
  // launch began, so the test is uniform over the grid -- every workgroup leaves before it touches a queue counter, and counters
  // nobody touched are still the zeros the next launch relies on.
  if (p.n_frames_dev && q_load(p.n_frames_dev) <= 0) return;
  BB_STATE st(p, smem);
  const int tid = threadIdx.x;
  const FrameQueues& q = p.q;
  // software pipeline over the frames: while frame k is searched, frame k + 1 has been pulled from the queue (one frame
  // per pull: frames of this size are never cheap enough for the queue atomic to matter) and is on its way from HBM
  // into the spare LDS buffer
  if (tid == 0) {
    const int it = q_add(&q.counters[QC_NEXT_FRAME], 1);
    st.misc[MI_ITEM] = it < frame_count(p) ? it : -1;
  }
  if (tid < 10) st.bt[(size_t)st.cn() * st.M * 10 + tid] = 0.0;  // the table's record of zeros (never overwritten)
  __syncthreads();
  int item = st.misc[MI_ITEM];
  if (item >= 0) st.prefetch_lds(item);
  wait_own_stores();
  __syncthreads();
  st.pc_start();  // (the measuring build's phase clocks, BBState::pc_mark: empty otherwise)
  while (item >= 0) {
    const int64_t frame = item;
    bb_prio<kPrioPhase>();
    st.stage(frame);
    st.template pc_mark<BB_STATE::PC_OTHER>();  // the frame's last barrier to its first: the swap, the status stores, the loop
    st.match();
    bb_prio<kPrioEval>();
    const int next = st.misc[MI_NEXT];
    if (next >= 0) st.prefetch_lds(next);  // in flight until the search's entry (BBState::search) or the frame's last barrier
    if (tid == 0) {
      const int status = st.misc[MI_STATUS];
      p.n_out[frame] = status ? 0 : st.misc[MI_NOUT];
      p.status[frame] = status;
      if (p.n_cand) p.n_cand[frame] = st.misc[MI_G];
    }
    const uint32_t G = (uint32_t)st.misc[MI_G];
    if (G) {
      // the bound tests pay their fixed cost (seed pass + a test per block) only on frames with enough candidates;
      // smaller frames queue every block -- same evaluation rounds, same result
      st.search(G >= (uint32_t)p.bb_min_g);
      bb_prio<kPrioPhase>();
      const int nroots = st.misc[MI_NROOTS];
      st.fresh_tid();
      for (int r = st.tid; r < nroots; r += kBBThreads) {
        if (st.outslot[r] >= 0) st.write_point(frame, r);  // (a root with candidates: only those have an output slot)
      }
    }
    wait_own_stores();  // ... and loads: the next frame's blobs are in LDS
    bb_prio<kPrioEval>();
    __syncthreads();  // the frame's LDS state is dead: the next one may be staged
    st.template pc_mark<BB_STATE::PC_PHASE_E>();  // ... with the search's last wait and barrier (the winners' records are in L2)
    item = next;
  }
  st.pc_flush();
  // the last workgroup to leave puts the queue counters back to zero: the next launch needs no memset
  if (tid == 0 && q_add(&q.counters[QC_EXITED], 1) == (int)gridDim.x - 1)
    for (int c = 0; c < QC_COUNT; c++) q_store(&q.counters[c], 0);
