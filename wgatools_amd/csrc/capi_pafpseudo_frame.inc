/* capi_pafpseudo_frame.inc — K31: the row frame writer of `pafpseudo` (wga_k31_pseudo_frame.h).
 * A part of wga_capi.cpp (included there: one translation unit). */
extern "C" {

int wga_pafpseudo_frame(wga_ctx* c, uint64_t n_items, const wga_span_item* d_items, const uint8_t* d_pool, uint64_t pool_bytes,
                        const uint8_t* d_text, uint64_t text_bytes, uint8_t* d_out, uint64_t out_bytes, uint64_t* d_first_bad) {
  static_assert(sizeof(wga_span_item) == 32, "K31's item layout");
  int rc = ctx_bind(c);
  if (rc) return rc;
  if (!d_first_bad) return fail(WGA_E_INVALID_ARG, "d_first_bad null", nullptr);
  if (n_items && (!d_items || !d_out)) return fail(WGA_E_INVALID_ARG, "null array", nullptr);
  if ((pool_bytes && !d_pool) || (text_bytes && !d_text)) return fail(WGA_E_INVALID_ARG, "null source", nullptr);
  if ((uintptr_t)d_out & 15u) return fail(WGA_E_INVALID_ARG, "d_out not 16-byte aligned", nullptr);
  if (n_items == 0 && out_bytes) return fail(WGA_E_INVALID_ARG, "no items for a text with bytes", nullptr);
  if (out_bytes >> 47) return fail(WGA_E_INVALID_ARG, "text too large for one launch", nullptr);
  if (n_items >> 39) return fail(WGA_E_INVALID_ARG, "too many items for one launch", nullptr);
  RT_CHECK(rt_memset(d_first_bad, 0xFF, sizeof(u64), c->stream));
  if (n_items == 0) return WGA_OK;
  WGA_LAUNCH(k_pseudo_frame_check, (u32)((n_items + 255u) / 256u), WGA_BLOCK, c->stream, (u64)n_items, d_items, (u64)pool_bytes,
             (u64)text_bytes, (u64)out_bytes, (u64*)d_first_bad);
  LAUNCH_CHECK();
  if (out_bytes == 0) return WGA_OK;
  WGA_LAUNCH(k_pseudo_frame_fill, (u32)((out_bytes + WGA_PSEUDO_FRAME_TILE - 1u) / WGA_PSEUDO_FRAME_TILE), WGA_BLOCK, c->stream,
             (u64)n_items, d_items, d_pool, d_text, d_out, (const u64*)d_first_bad);
  LAUNCH_CHECK();
  return WGA_OK;
}

} /* extern "C" */
