/* capi_multigpu.inc — the reduce-scatter across devices.
 * A part of wga_capi.cpp (included there: one translation unit). */
extern "C" {

int wga_reduce_scatter_i32(wga_ctx** ctxs, int ngpu, int32_t** d_bufs, uint64_t count) {
  if (!ctxs || !d_bufs || ngpu < 1) return fail(WGA_E_INVALID_ARG, "null argument", nullptr);
  for (int g = 0; g < ngpu; g++) {
    if (!ctxs[g] || (count && !d_bufs[g])) return fail(WGA_E_INVALID_ARG, "null context / buffer", nullptr);
    for (int h = 0; h < g; h++)
      if (ctxs[h] == ctxs[g] || (!ctxs[0]->rs_same_device_ok && ctxs[h]->device == ctxs[g]->device))
        return fail(WGA_E_INVALID_ARG, "two contexts on one device", nullptr);
  }
  if (ngpu == 1 || count == 0) return WGA_OK;
  int rc;
  /* Nothing here waits on the host.  (1) every context records "my buffer is as my stream leaves it"; (2) device g's stream
   * waits for the others' records and adds their slices g to its own — read where they lie, by ONE kernel that has a load
   * per peer in flight in every thread (all of the device's xGMI links carry data at once), or, without peer access, pulled
   * into scratch by N-1 copies on N-1 streams of their own (in flight together as well) and added by the same kernel;
   * (3) every context's stream waits until the others have read its buffer.  Work enqueued behind the call on any of the
   * contexts' streams sees the result. */
  for (int g = 0; g < ngpu; g++) {
    wga_ctx* c = ctxs[g];
    if ((rc = ctx_bind(c))) return rc;
    if (!c->rs_have_ev) {
      RT_CHECK(rt_event_create(&c->rs_ready));
      RT_CHECK(rt_event_create(&c->rs_done));
      c->rs_have_ev = true;
    }
    RT_CHECK(rt_event_record(c->rs_ready, c->stream));
  }
  bool direct = true;
  for (int g = 0; g < ngpu && direct; g++) {
    if (ctxs[g]->rs_staged) direct = false;
    for (int h = 0; h < ngpu && direct; h++)
      if (h != g && rt_peer_enable(ctxs[g]->device, ctxs[h]->device)) direct = false;
  }
  for (int g = 0; g < ngpu; g++) {
    wga_ctx* c = ctxs[g];
    const u64 lo = count * (u64)g / (u64)ngpu, hi = count * (u64)(g + 1) / (u64)ngpu, n = hi - lo;
    if ((rc = ctx_bind(c))) return rc;
    if (n) {
      int* stage = nullptr;
      if (!direct) {
        void* ws;
        if ((rc = ctx_scratch(c, (size_t)n * 4 * (size_t)(ngpu - 1), &ws))) return rc;
        stage = (int*)ws;
        while ((int)c->rs_streams.size() < ngpu - 1) {
          wga_stream_t st;
          rt_event_t ev;
          RT_CHECK(rt_stream_create(&st));
          c->rs_streams.push_back(st);
          RT_CHECK(rt_event_create(&ev));
          c->rs_copied.push_back(ev);
        }
      }
      const u32 grid = (u32)(n / 1024u < 16384u ? (n + 1023u) / 1024u : 16384u);
      int k = 0;
      wga_peer_srcs srcs;
      int n_src = 0;
      auto add = [&]() {
        WGA_LAUNCH(k_add_peers_i32, grid, WGA_BLOCK, c->stream, (int*)d_bufs[g] + lo, srcs, n_src, (u64)n);
        n_src = 0;
      };
      for (int h = 0; h < ngpu; h++) {
        if (h == g) continue;
        if (direct) {
          RT_CHECK(rt_stream_wait_event(c->stream, ctxs[h]->rs_ready));
          srcs.p[n_src++] = (const int*)d_bufs[h] + lo;
        } else { /* the scratch is this stream's: the pull starts behind what the stream had in flight, on a stream of its own */
          wga_stream_t st = c->rs_streams[k];
          RT_CHECK(rt_stream_wait_event(st, c->rs_ready));
          RT_CHECK(rt_stream_wait_event(st, ctxs[h]->rs_ready));
          RT_CHECK(rt_peer_copy(stage + (size_t)k * n, c->device, d_bufs[h] + lo, ctxs[h]->device, (size_t)n * 4, st));
          RT_CHECK(rt_event_record(c->rs_copied[k], st)); /* the staged pieces are named below, WGA_PEER_MAX per launch */
        }
        k++;
        if (n_src == WGA_PEER_MAX && direct) { /* more peers than one launch takes (never on one node) */
          add();
          LAUNCH_CHECK();
        }
      }
      if (!direct) {
        /* every pull has been enqueued — they run side by side — and only now does the adding stream wait for them */
        for (int j = 0; j < k; j++) RT_CHECK(rt_stream_wait_event(c->stream, c->rs_copied[j]));
        for (int j0 = 0; j0 < k; j0 += WGA_PEER_MAX) {
          n_src = 0;
          for (int j = j0; j < k && j < j0 + WGA_PEER_MAX; j++) srcs.p[n_src++] = stage + (size_t)j * n;
          add();
          LAUNCH_CHECK();
        }
      } else if (n_src) {
        add();
        LAUNCH_CHECK();
      }
    }
    RT_CHECK(rt_event_record(c->rs_done, c->stream));
  }
  for (int h = 0; h < ngpu; h++) {
    if ((rc = ctx_bind(ctxs[h]))) return rc;
    for (int g = 0; g < ngpu; g++)
      if (g != h) RT_CHECK(rt_stream_wait_event(ctxs[h]->stream, ctxs[g]->rs_done));
  }
  return WGA_OK;
}

#ifdef WGA_EMU
/* test hook of the emulator build only (not part of the ABI): the most peer copies that were outstanding towards `device` at
 * one time, as the emulator's streams keep the book (wga_rt.h) */
int wga_emu_peer_copies_in_flight(int device) { return emu_book().most[device & 63]; }
void wga_emu_peer_copies_reset(void) { emu_book() = emu_peer_book(); }
#endif

} /* extern "C" */
