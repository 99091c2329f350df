"""Thin object layer over the C-ABI: device arrays and one method per entry point.

No computation happens here — every method forwards to libwgahip.so.  Arrays live in HBM
(`DeviceArray`); `upload` / `numpy()` are the only host<->device copies.
"""
import ctypes as C

import numpy as np

from . import _lib

COUNTS_DTYPE = np.dtype([(k, "<u8") for k in (
    "match", "mismatch", "ins_ev", "ins_bp", "del_ev", "del_bp", "inv_ins_ev", "inv_ins_bp",
    "inv_del_ev", "inv_del_bp", "inv_ev")])
DIAG_DTYPE = np.dtype([("bad_op_idx", "<u8"), ("panic_op_idx", "<u8"), ("bad_base_pos", "<u8")])
CHAIN_TRIM_DTYPE = np.dtype([(k, "<u8") for k in ("head_ins", "head_del", "tail_ins", "tail_del")])
TOK_ERR_DTYPE = np.dtype([("err", np.int32), ("tok_len", np.uint32), ("tok_off", np.uint64)])
CLASS_SUMS_DTYPE = np.dtype([(k, "<u8") for k in ("mx", "i", "d", "s", "o")])
FA_CONTIG_DTYPE = np.dtype([(k, "<u8") for k in ("hdr_start", "hdr_end", "pool_off", "len")])
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MAF_LINE_DTYPE = np.dtype([("num", np.uint64, 3), ("name_off", np.uint64), ("seq_off", np.uint64),
                           ("seq_len", np.uint64), ("name_len", np.uint32), ("strand_neg", np.uint8),
                           ("status", np.uint8), ("pad", np.uint8, 2)])
PAF_LINE_DTYPE = np.dtype([("num", np.uint64, 9), ("qname_off", np.uint64), ("tname_off", np.uint64),
                           ("cg_beg", np.uint64), ("cg_end", np.uint64), ("qname_len", np.uint32),
                           ("tname_len", np.uint32), ("n_fields", np.uint32), ("strand_neg", np.uint8),
                           ("status", np.uint8), ("pad", np.uint8, 2)])
CHAIN_HEAD_DTYPE = np.dtype([("num", np.uint64, 8), ("tname_off", np.uint64), ("qname_off", np.uint64),
                             ("tname_len", np.uint32), ("qname_len", np.uint32), ("tstrand_neg", np.uint8),
                             ("qstrand_neg", np.uint8), ("pad", np.uint8, 6)])
CHAIN_OK, CHAIN_FALLBACK = 0, 1
# K24 (include/wga_hip.h wga_paf_pair / wga_paf_filter_params; WGA_PAF_FILTER_TILE_BYTES)
PAF_PAIR_DTYPE = np.dtype([("first_line", "<u8"), ("sum", "<u8"), ("qname_off", "<u8"), ("tname_off", "<u8"),
                           ("qname_len", "<u4"), ("tname_len", "<u4")])
PAF_FILTER_PARAMS_DTYPE = np.dtype([("min_block_size", "<u8"), ("min_query_size", "<u8"), ("d_pair_of_line", "<u8"),
                                    ("d_pair_keep", "<u8")])
PAF_OK, PAF_SKIP, PAF_FALLBACK = 0, 1, 2
PAF_FILTER_TILE = 8192
# K29 (include/wga_hip.h wga_paf_fix_sizes; WGA_PAF_FIX_TILE_BYTES)
PAF_FIX_SIZES_DTYPE = np.dtype([(k, "<u8") for k in ("rows_bytes", "qlist_bytes", "tlist_bytes", "n_records", "n_q_bad", "n_t_bad")])
PAF_FIX_TILE = 8192
# K25 (include/wga_hip.h wga_chain_filter_params)
CHAIN_FILTER_PARAMS_DTYPE = np.dtype([("min_block_size", "<u8"), ("min_query_size", "<u8")])
# K28 (include/wga_hip.h wga_maf2paf_head)
MAF2PAF_HEAD_DTYPE = np.dtype([("q", np.uint64, 3), ("t", np.uint64, 3), ("qname_off", np.uint64), ("tname_off", np.uint64),
                               ("qname_len", np.uint32), ("tname_len", np.uint32), ("strand_neg", np.uint8),
                               ("pad", np.uint8, 7)])
# K31 (include/wga_hip.h wga_span_item, WGA_SPAN_*, WGA_PSEUDO_FRAME_TILE)
SPAN_ITEM_DTYPE = np.dtype([("dst", "<u8"), ("len", "<u8"), ("src", "<u8"), ("kind", "<u4"), ("pad", "<u4")])
SPAN_FILL, SPAN_COPY_POOL, SPAN_COPY_TEXT, SPAN_HOLE = 0, 1, 2, 3
PSEUDO_FRAME_TILE = 65536
# K33 (include/wga_hip.h wga_stat_row_head)
STAT_ROW_HEAD_DTYPE = np.dtype([("ref_size", "<u8"), ("ref_start", "<u8"), ("query_size", "<u8"), ("query_start", "<u8"),
                                ("rname_off", "<u8"), ("qname_off", "<u8"), ("rname_len", "<u4"), ("qname_len", "<u4")])
assert STAT_ROW_HEAD_DTYPE.itemsize == 56
# K34 (include/wga_hip.h wga_dotplot_ov_head)
DOTPLOT_OV_HEAD_DTYPE = np.dtype([("ref_start", "<u8"), ("ref_end", "<u8"), ("q_first", "<u8"), ("q_second", "<u8"),
                                  ("align_size", "<u8"), ("rname_off", "<u8"), ("qname_off", "<u8"), ("rname_len", "<u4"),
                                  ("qname_len", "<u4")])
assert DOTPLOT_OV_HEAD_DTYPE.itemsize == 64
# K35 (include/wga_hip.h wga_maf_index_name, WGA_E_FALLBACK)
MAF_INDEX_NAME_DTYPE = np.dtype([("name_off", "<u8"), ("size", "<u8"), ("first_line", "<u8"), ("n_ivls", "<u8"), ("text_off", "<u8"),
                                 ("name_len", "<u4"), ("isref", "<u4")])
assert MAF_INDEX_NAME_DTYPE.itemsize == 48
E_FALLBACK = -6
# K36 (include/wga_hip.h wga_stat_pair)
STAT_PAIR_DTYPE = np.dtype([("first_rec", "<u8"), ("n_recs", "<u8"), ("ref_start", "<u8"), ("query_start", "<u8"),
                            ("sum", COUNTS_DTYPE), ("inv_size_bits", "<u4"), ("pad", "<u4")])
assert STAT_PAIR_DTYPE.itemsize == 128
# K32 (include/wga_hip.h wga_maf_frame_head)
MAF_FRAME_HEAD_DTYPE = np.dtype([("score", "<u8"), ("t", np.uint64, 3), ("q", np.uint64, 3), ("tname_off", "<u8"),
                                 ("qname_off", "<u8"), ("tname_len", "<u4"), ("qname_len", "<u4"), ("t_neg", np.uint8),
                                 ("q_neg", np.uint8), ("pad", np.uint8, 6)])

OP_CODES = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
OP_I_CONT, OP_D_CONT, OP_OTHER = 9, 10, 11
OP_MAX_LEN = (1 << 28) - 1

REC_ERR_NAMES = {0: "ok", 1: "CigarTagNotFound", 2: "CigarOpInvalid", 3: "ParseIntError",
                 4: "InvalidBase", 5: "NomErr", 6: "panic"}


class DeviceArray:
    """A typed view of an HBM allocation owned by (or borrowed into) an Engine."""

    def __init__(self, eng, ptr, shape, dtype, owner=True):
        self.eng = eng
        self.ptr = ptr
        self.shape = tuple(shape) if not np.isscalar(shape) else (int(shape),)
        self.dtype = np.dtype(dtype)
        self.owner = owner

    @property
    def size(self):
        return int(np.prod(self.shape)) if self.shape else 1

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        self.eng._check(self.eng.lib.wga_memcpy_d2h(self.eng.ctx, out.ctypes.data, self.ptr,
                                                    self.nbytes))
        return out

    def fill(self, byte):
        self.eng._check(self.eng.lib.wga_memset(self.eng.ctx, self.ptr, byte, self.nbytes))
        return self

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (int(self.ptr), False), "version": 2,
                "strides": None}

    def torch(self, device):
        """zero-copy torch view of this allocation (plumbing for the harness: torch only sees the bytes); the
        DeviceArray must outlive the tensor"""
        import torch
        t = torch.as_tensor(self, device=device)
        if t.data_ptr() != int(self.ptr):
            raise RuntimeError("torch copied the buffer instead of viewing it")
        return t

    def free(self):
        if self.owner and self.ptr:
            self.eng.lib.wga_free(self.eng.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _p(x):
    """device pointer of a DeviceArray / torch tensor / int / None"""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class Batch:
    """A device-resident CSR batch of packed CIGARs (wga_cigar_batch)."""

    def __init__(self, ops, op_off, strand_neg, n, n_ops):
        self.ops, self.op_off, self.strand_neg = ops, op_off, strand_neg
        self.n, self.n_ops = int(n), int(n_ops)
        self.c = _lib.CigarBatch(_p(ops), _p(op_off), _p(strand_neg), self.n_ops, self.n)


# K20 tables (include/wga_hip.h wga_maf_chunk_row / wga_maf_chunk_block)
MAF_CHUNK_ROW_DTYPE = np.dtype([("seq_off", "<u8"), ("seq_len", "<u8"), ("name_off", "<u8"), ("start", "<u8"),
                                ("src_size", "<u8"), ("name_len", "<u4"), ("strand_neg", "<u4")])
MAF_CHUNK_BLOCK_DTYPE = np.dtype([("row0", "<u8"), ("k_lo", "<u8"), ("k_hi", "<u8"), ("n_rows", "<u4"), ("pad", "<u4")])
# K21 tables (include/wga_hip.h wga_maf_slice_row / wga_maf_slice_hit)
MAF_SLICE_ROW_DTYPE = np.dtype([("seq_off", "<u8"), ("seq_len", "<u8"), ("name_off", "<u8"), ("start", "<u8"), ("size", "<u8"),
                                ("src_size", "<u8"), ("name_len", "<u4"), ("strand_neg", "<u4")])
MAF_SLICE_HIT_DTYPE = np.dtype([("row0", "<u8"), ("cut_lo", "<u8"), ("cut_hi", "<u8"), ("n_rows", "<u4"), ("ord", "<u4"),
                                ("whole", "<u4"), ("pad", "<u4")])
# K22 tables (include/wga_hip.h wga_maf_rewrite_block / wga_maf_rewrite_params; the rows are K21's)
MAF_REWRITE_BLOCK_DTYPE = np.dtype([("row0", "<u8"), ("n_rows", "<u4"), ("pad", "<u4")])
MAF_REWRITE_PARAMS_DTYPE = np.dtype([("min_block_size", "<u8"), ("min_query_size", "<u8"), ("filter", "<u4"), ("n_prefix", "<u4"),
                                     ("d_prefix_text", "<u8"), ("d_prefix_off", "<u8")])
VCF_ERR_DTYPE = np.dtype([("item", "<u8"), ("kind", "<u4"), ("ch", "<u4")])
VCF_REC_DTYPE = np.dtype([("t_name_off", "<u8"), ("q_name_off", "<u8"), ("t_name_len", "<u4"), ("q_name_len", "<u4"),
                          ("t_start", "<u8"), ("t_end", "<u8"), ("q_start", "<u8"), ("q_end", "<u8"),
                          ("t_off", "<u8"), ("t_len", "<u8"), ("q_off", "<u8"), ("q_len", "<u8")])
MAF_VCF_REC_DTYPE = np.dtype([("t_name_off", "<u8"), ("q_name_off", "<u8"), ("t_name_len", "<u4"), ("q_name_len", "<u4"),
                              ("t_start", "<u8"), ("q_start", "<u8"), ("q_size", "<u8"), ("q_neg", "<u4"), ("pad", "<u4")])


class Engine:
    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None else _lib.load()
        ctx = C.c_void_p()
        rc = self.lib.wga_ctx_create(device, C.byref(ctx))
        if rc != 0:
            raise _lib.WgaError("wga_ctx_create failed (%d): %s" % (
                rc, self.lib.wga_last_error().decode()))
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.wga_ctx_destroy(self.ctx)
            self.ctx = None

    def _check(self, rc):
        if rc != 0:
            raise _lib.WgaError("libwgahip call failed (%d): %s" % (
                rc, self.lib.wga_last_error().decode()))

    # ---- memory -----------------------------------------------------------------------------
    def empty(self, shape, dtype):
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) if not np.isscalar(shape) else int(shape)
        ptr = C.c_void_p()
        self._check(self.lib.wga_malloc(self.ctx, max(n * dt.itemsize, 16), C.byref(ptr)))
        return DeviceArray(self, ptr.value, shape, dt)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.empty(arr.shape, arr.dtype)
        self._check(self.lib.wga_memcpy_h2d(self.ctx, d.ptr, arr.ctypes.data, arr.nbytes))
        self.sync()  # the host array may be a temporary
        return d

    def copy_into(self, dst, arr):
        """host array -> an existing device array (the same pointer keeps its address)"""
        arr = np.ascontiguousarray(arr)
        self._check(self.lib.wga_memcpy_h2d(self.ctx, dst.ptr, arr.ctypes.data, arr.nbytes))
        self.sync()

    def download_slice(self, src, byte_off, nbytes):
        """bytes [byte_off, byte_off + nbytes) of a device array (or of a device pointer) as a numpy array of u8"""
        out = np.empty(int(nbytes), dtype=np.uint8)
        if nbytes:
            self._check(self.lib.wga_memcpy_d2h(self.ctx, out.ctypes.data, _p(src) + int(byte_off), int(nbytes)))
        return out

    def sync(self):
        self._check(self.lib.wga_sync(self.ctx))

    def set_stream(self, hip_stream):
        """launch on this hipStream_t (0 / None = HIP's default stream)"""
        self._check(self.lib.wga_ctx_set_stream(self.ctx, hip_stream or None))

    def reset_stream(self):
        self._check(self.lib.wga_ctx_reset_stream(self.ctx))

    def set_param(self, name, value):
        self._check(self.lib.wga_ctx_set_param(self.ctx, name.encode(), int(value)))

    def get_param(self, name):
        v = C.c_int64(0)
        self._check(self.lib.wga_ctx_get_param(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def expand_timing(self):
        """(summed ms, launches) of the expand kernel proper since the last call ("expand_timing" param)"""
        ms, n = C.c_double(0.0), C.c_uint32(0)
        self._check(self.lib.wga_ctx_expand_timing(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- host packer ------------------------------------------------------------------------
    def pack_cigar(self, text):
        """CIGAR text (after 'cg:Z:') -> (ops u32[], err code, (tok_off, tok_len))."""
        if isinstance(text, str):
            text = text.encode()
        n = C.c_size_t()
        err = C.c_int32()
        eo, el = C.c_size_t(), C.c_size_t()
        cap = max(1, text.count(b"M") + len(text))  # generous first guess
        ops = np.empty(cap, dtype=np.uint32)
        rc = self.lib.wga_cigar_pack(text, len(text), ops.ctypes.data, cap, C.byref(n),
                                     C.byref(err), C.byref(eo), C.byref(el))
        if rc == -5:  # WGA_E_TOO_SMALL
            cap = n.value
            ops = np.empty(cap, dtype=np.uint32)
            rc = self.lib.wga_cigar_pack(text, len(text), ops.ctypes.data, cap, C.byref(n),
                                         C.byref(err), C.byref(eo), C.byref(el))
        self._check(rc)
        return ops[: n.value].copy(), err.value, (eo.value, el.value)

    def make_batch(self, ops, op_off, strand_neg):
        """numpy CSR arrays -> device Batch"""
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        op_off = np.ascontiguousarray(op_off, dtype=np.uint64)
        strand_neg = np.ascontiguousarray(strand_neg, dtype=np.uint8)
        n = len(strand_neg)
        assert len(op_off) == n + 1 and int(op_off[-1]) == len(ops)
        return Batch(self.upload(ops), self.upload(op_off), self.upload(strand_neg), n, len(ops))

    def make_batch_device(self, ops, op_off, strand_neg, n, n_ops):
        """device arrays (e.g. written by the tokeniser or the K11 bridges) -> Batch"""
        return Batch(ops, op_off, strand_neg, int(n), int(n_ops))

    # ---- kernels ----------------------------------------------------------------------------
    def tile_ws(self, n_ops):
        return self.empty(self.lib.wga_tile_ws_bytes(int(n_ops)), np.uint8)

    def cigar_stat(self, batch, counts=None, diag=None, tile_ws=None, want_tiles=True):
        counts = counts if counts is not None else self.empty(batch.n, COUNTS_DTYPE)
        diag = diag if diag is not None else self.empty(batch.n, DIAG_DTYPE)
        if tile_ws is None and want_tiles:
            tile_ws = self.tile_ws(batch.n_ops)
        self._check(self.lib.wga_cigar_stat(self.ctx, C.byref(batch.c), _p(counts), _p(diag),
                                            _p(tile_ws)))
        return counts, diag, tile_ws

    def cigar_class_sums(self, batch, sums=None):
        sums = sums if sums is not None else self.empty(batch.n, CLASS_SUMS_DTYPE)
        self._check(self.lib.wga_cigar_class_sums(self.ctx, C.byref(batch.c), _p(sums)))
        return sums

    def paf2maf_layout(self, n, counts, t_src_len, q_src_len, pre_t=None, pre_q=None, post=None,
                       t_row_off=None, q_row_off=None, rec_off=None):
        t_row_off = t_row_off if t_row_off is not None else self.empty(n, np.uint64)
        q_row_off = q_row_off if q_row_off is not None else self.empty(n, np.uint64)
        rec_off = rec_off if rec_off is not None else self.empty(n + 1, np.uint64)
        self._check(self.lib.wga_paf2maf_layout(self.ctx, n, _p(counts), _p(t_src_len),
                                                _p(q_src_len), _p(pre_t), _p(pre_q), _p(post),
                                                _p(t_row_off), _p(q_row_off), _p(rec_off)))
        return t_row_off, q_row_off, rec_off

    def paf2maf_expand(self, batch, counts, tile_ws, t_fa, t_fa_bytes, t_src_off, t_src_len, q_fa,
                       q_fa_bytes, q_src_off, q_src_len, out, t_row_off, q_row_off, diag):
        self._check(self.lib.wga_paf2maf_expand(
            self.ctx, C.byref(batch.c), _p(counts), _p(tile_ws), _p(t_fa), int(t_fa_bytes),
            _p(t_src_off), _p(t_src_len), _p(q_fa), int(q_fa_bytes), _p(q_src_off), _p(q_src_len),
            _p(out), _p(t_row_off), _p(q_row_off), _p(diag)))

    def bgzf_inflate(self, d_in, in_bytes, n_blocks, blocks, out, status):
        """BGZF members inflated on the device (wga_bgzf_inflate); blocks: n x (in_off u64, in_len u32, out_len u32, out_off u64)"""
        self._check(self.lib.wga_bgzf_inflate(self.ctx, _p(d_in), int(in_bytes), int(n_blocks), _p(blocks), _p(out), _p(status)))

    def bgzf_crc32(self, text, n_blocks, blocks, crc):
        """CRC-32 of every member's inflated bytes (wga_bgzf_crc32); blocks as for bgzf_inflate, crc: n x u32"""
        self._check(self.lib.wga_bgzf_crc32(self.ctx, _p(text), int(n_blocks), _p(blocks), _p(crc)))

    def bgzf_compress(self, d_in, n_bytes, out=None, eof_marker=True, in_offset=0, out_offset=0, out_cap=None):
        """bytes in HBM -> BGZF members (wga_bgzf_compress, K18); returns (DeviceArray of the worst-case size, bytes used).
        in_offset / out_offset: byte offsets into d_in / out (any alignment).  The capacity handed to the library is what `out`
        really holds behind out_offset (a DeviceArray's or a tensor's own size; out_cap for a raw pointer): the library's
        own check then refuses a buffer that is too small instead of writing past it."""
        cap = int(self.lib.wga_bgzf_bound(int(n_bytes)))
        if out is None:
            out = self.empty(cap + int(out_offset), np.uint8)
        if out_cap is None:
            if isinstance(out, DeviceArray):
                out_cap = out.nbytes - int(out_offset)
            elif hasattr(out, "numel") and hasattr(out, "element_size"):
                out_cap = out.numel() * out.element_size() - int(out_offset)
            else:
                raise ValueError("bgzf_compress: out_cap is required when `out` is a raw pointer")
        if out_cap < 0:
            raise ValueError("bgzf_compress: out_offset lies behind the end of `out`")
        used = C.c_uint64(0)
        src = _p(d_in)
        self._check(self.lib.wga_bgzf_compress(self.ctx, (src + int(in_offset)) if src else None, int(n_bytes),
                                               _p(out) + int(out_offset), int(out_cap), C.byref(used), 1 if eof_marker else 0))
        return out, int(used.value)

    def scatter_bytes(self, n, src, src_off, dst, dst_off):
        self._check(self.lib.wga_scatter_bytes(self.ctx, n, _p(src), _p(src_off), _p(dst),
                                               _p(dst_off)))

    def exclusive_scan_u64(self, n, d_in, d_out=None):
        d_out = d_out if d_out is not None else self.empty(n + 1, np.uint64)
        self._check(self.lib.wga_exclusive_scan_u64(self.ctx, n, _p(d_in), _p(d_out)))
        return d_out

    def maf_pair_stat(self, n, rows, t_off, q_off, cols, strand_neg, counts=None, run_cnt=None,
                      runs=None, run_off=None):
        counts = counts if counts is not None else self.empty(n, COUNTS_DTYPE)
        run_cnt = run_cnt if run_cnt is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_maf_pair_stat(self.ctx, n, _p(rows), _p(t_off), _p(q_off),
                                               _p(cols), _p(strand_neg), _p(counts), _p(run_cnt),
                                               _p(runs), _p(run_off)))
        return counts, run_cnt

    def maf_call_runs(self, n, rows, t_off, q_off, cols, run_cnt=None, runs=None, run_off=None):
        run_cnt = run_cnt if run_cnt is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_maf_call_runs(self.ctx, n, _p(rows), _p(t_off), _p(q_off), _p(cols),
                                               _p(run_cnt), _p(runs), _p(run_off)))
        return run_cnt

    def maf_call_vcf(self, n, rows, t_off, q_off, cols, runs, run_off, recs, names, snp, inv, svlen, chunk_size,
                     nbytes=None, err=None, out=None, out_off=None):
        """the rules and VCF rows of `call` on MAF (wga_maf_call_vcf, K19) on K4's run list: count pass when out is None
        (returns nbytes, err), fill pass otherwise.  recs: n x MAF_VCF_REC_DTYPE"""
        if out is None:
            nbytes = nbytes if nbytes is not None else self.empty(n, np.uint64)
            err = err if err is not None else self.empty(n, VCF_ERR_DTYPE)
        self._check(self.lib.wga_maf_call_vcf(self.ctx, n, _p(rows), _p(t_off), _p(q_off), _p(cols), _p(runs), _p(run_off),
                                              _p(recs), _p(names), 1 if snp else 0, 1 if inv else 0, int(svlen), int(chunk_size),
                                              _p(nbytes) if out is None else None, _p(err) if out is None else None,
                                              _p(out), _p(out_off)))
        return nbytes, err

    def cigar_tokenise(self, n, text, text_off, op_cnt=None, err=None, ops=None, op_off=None):
        """device tokeniser (wga_cigar_tokenise): count pass when ops is None, fill pass otherwise"""
        op_cnt = op_cnt if op_cnt is not None else self.empty(n, np.uint64)
        err = err if err is not None else self.empty(n, TOK_ERR_DTYPE)
        self._check(self.lib.wga_cigar_tokenise(self.ctx, n, _p(text), _p(text_off), _p(op_cnt), _p(err),
                                                _p(ops), _p(op_off)))
        return op_cnt, err

    def cigar_chain(self, batch, trim=None, nbytes=None, diag=None, out=None, out_off=None):
        """paf2chain data lines: count pass when out is None (trim, nbytes, diag), fill pass otherwise"""
        if out is None:
            trim = trim if trim is not None else self.empty(batch.n, CHAIN_TRIM_DTYPE)
            nbytes = nbytes if nbytes is not None else self.empty(batch.n, np.uint64)
            diag = diag if diag is not None else self.empty(batch.n, DIAG_DTYPE)
        self._check(self.lib.wga_cigar_chain(self.ctx, C.byref(batch.c), _p(trim), _p(nbytes), _p(diag),
                                             _p(out), _p(out_off)))
        return trim, nbytes, diag

    def maf_runs_ops(self, n, n_elems, runs, run_off, cols, cnt=None, out=None, out_off=None):
        """K3 runs -> packed ops (count pass when out is None)"""
        cnt = cnt if cnt is not None or out is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_maf_runs_ops(self.ctx, n, int(n_elems), _p(runs), _p(run_off), _p(cols),
                                              _p(cnt), _p(out), _p(out_off)))
        return cnt

    def maf_runs_cigar_text(self, n, n_elems, runs, run_off, cols, cnt=None, out=None, out_off=None):
        """K3 runs -> maf2paf's cg:Z: text (count pass when out is None)"""
        cnt = cnt if cnt is not None or out is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_maf_runs_cigar_text(self.ctx, n, int(n_elems), _p(runs), _p(run_off),
                                                     _p(cols), _p(cnt), _p(out), _p(out_off)))
        return cnt

    def chain_lines_ops(self, n, n_elems, lines, line_off, cnt=None, out=None, out_off=None):
        """chain data lines (size, D, I) -> packed ops (count pass when out is None)"""
        cnt = cnt if cnt is not None or out is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_chain_lines_ops(self.ctx, n, int(n_elems), _p(lines), _p(line_off), _p(cnt),
                                                 _p(out), _p(out_off)))
        return cnt

    def chain_lines_cigar_text(self, n, n_elems, lines, line_off, cnt=None, out=None, out_off=None):
        """chain data lines -> chain2paf's CIGAR text (count pass when out is None)"""
        cnt = cnt if cnt is not None or out is not None else self.empty(n, np.uint64)
        self._check(self.lib.wga_chain_lines_cigar_text(self.ctx, n, int(n_elems), _p(lines), _p(line_off),
                                                        _p(cnt), _p(out), _p(out_off)))
        return cnt

    def cigar_dotplot(self, batch, cutoff, t_start, q_start, seg_cnt=None, segs=None, seg_off=None):
        """dotplot base-level segments (5 u64 each): count pass when segs is None"""
        seg_cnt = seg_cnt if seg_cnt is not None or segs is not None else self.empty(batch.n, np.uint64)
        self._check(self.lib.wga_cigar_dotplot(self.ctx, C.byref(batch.c), int(cutoff), _p(t_start), _p(q_start),
                                               _p(seg_cnt), _p(segs), _p(seg_off)))
        return seg_cnt

    def paf_split(self, text, n_bytes, lines=None):
        """K13: number of text lines (lines is None), or the wga_paf_line of every line"""
        nl = C.c_uint64(0)
        cap = 0 if lines is None else (lines.numel() if hasattr(lines, "numel") else lines.size)
        self._check(self.lib.wga_paf_split(self.ctx, _p(text), int(n_bytes), C.byref(nl), _p(lines), int(cap)))
        return int(nl.value)

    def paf_pairs(self, text, n_bytes, lines, n_lines):
        """K24 (filter.rs:108-160): the (query name, target name) pairs of the OK lines of wga_paf_split's table, both calls
        of wga_paf_pairs.  Returns (pairs as numpy PAF_PAIR_DTYPE in first-line order, pair_of_line as a device array of u32:
        0xFFFFFFFF for a line that is not OK).  Bytes behind either array are checked to be left alone."""
        n_lines = int(n_lines)
        work = self.empty(max(int(self.lib.wga_paf_pairs_work_bytes(n_lines)), 16), np.uint8)
        np_ = C.c_uint64(0)
        args = (self.ctx, _p(text), int(n_bytes), _p(lines), n_lines, _p(work), C.byref(np_))
        self._check(self.lib.wga_paf_pairs(*args, None, None, 0))
        n_pairs = int(np_.value)
        pol = self.empty(n_lines + 4, np.uint32).fill(0xA5)
        pairs = self.empty(n_pairs + 1, PAF_PAIR_DTYPE).fill(0xA5)
        self._check(self.lib.wga_paf_pairs(*args, _p(pol), _p(pairs), n_pairs))
        self.sync()
        if int(np_.value) != n_pairs:
            raise _lib.WgaError("wga_paf_pairs changed *n_pairs in its second call")
        if not ((pol.numpy()[n_lines:] == 0xA5A5A5A5).all() and pairs.numpy()[n_pairs:].tobytes() == b"\xa5" * 40):
            raise _lib.WgaError("wga_paf_pairs wrote behind its arrays")
        pol.shape = (n_lines,)
        return pairs.numpy()[:n_pairs], pol

    def paf_filter(self, text, n_bytes, lines, n_lines, min_block_size=0, min_query_size=0, pair_of_line=None, pair_keep=None):
        """K24 (filter.rs:88-160): the text of the kept lines of wga_paf_split's table, both calls of wga_paf_filter.  Threshold
        mode, or pair mode when pair_keep (a device array of one byte per pair) and pair_of_line (wga_paf_pairs') are given.
        Returns (text, n_kept, first inexact line or None); the 64 bytes in front of and behind the text are checked."""
        n_lines = int(n_lines)
        par = np.zeros(1, dtype=PAF_FILTER_PARAMS_DTYPE)
        par["min_block_size"], par["min_query_size"] = int(min_block_size), int(min_query_size)
        if pair_keep is not None:
            par["d_pair_of_line"], par["d_pair_keep"] = _p(pair_of_line), _p(pair_keep)
        work = self.empty(max(int(self.lib.wga_paf_filter_work_bytes(n_lines)), 16), np.uint8)
        total, kept, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        args = (self.ctx, _p(text), int(n_bytes), _p(lines), n_lines, par.ctypes.data, _p(work), C.byref(total), C.byref(kept),
                C.byref(bad))
        self._check(self.lib.wga_paf_filter(*args, None))
        first = (int(total.value), int(kept.value), int(bad.value))
        guard = 64  # bytes around the text that the fill call must leave alone
        out = self.upload(np.full(first[0] + 2 * guard, 0xA5, dtype=np.uint8))
        self._check(self.lib.wga_paf_filter(*args, out.ptr + guard))
        self.sync()
        if (int(total.value), int(kept.value), int(bad.value)) != first:
            raise _lib.WgaError("wga_paf_filter changed its counts in the second call")
        got = out.numpy()
        if not ((got[:guard] == 0xA5).all() and (got[guard + first[0]:] == 0xA5).all()):
            raise _lib.WgaError("wga_paf_filter wrote outside d_out[0 .. text_bytes)")
        return got[guard:guard + first[0]].tobytes(), first[1], (None if first[2] == int(NONE) else first[2])

    def paf_fix_plan(self, text, n_bytes, lines, n_lines):
        """K29 (validate.rs:71-141): is the text of wga_paf_split's table taken, and where are its CIGARs: both calls of
        wga_paf_fix_plan.  Returns (n_records, first untaken line or None, cg_beg, cg_end as device arrays of u64); the
        words behind the two arrays, and all of them for an untaken text, are checked to be left alone."""
        n_lines = int(n_lines)
        work = self.empty(max(int(self.lib.wga_paf_fix_work_bytes(n_lines)), 16), np.uint8)
        nr, bad = C.c_uint64(0), C.c_uint64(0)
        args = (self.ctx, _p(text), int(n_bytes), _p(lines), n_lines, _p(work), C.byref(nr), C.byref(bad))
        self._check(self.lib.wga_paf_fix_plan(*args, None, None))
        first = (int(nr.value), int(bad.value))
        cap = first[0] if first[1] == int(NONE) else n_lines     # an untaken text: room the second call must not use
        beg = self.empty(cap + 2, np.uint64).fill(0xA5)
        end = self.empty(cap + 2, np.uint64).fill(0xA5)
        self._check(self.lib.wga_paf_fix_plan(*args, _p(beg), _p(end)))
        self.sync()
        if (int(nr.value), int(bad.value)) != first:
            raise _lib.WgaError("wga_paf_fix_plan changed its counts in the second call")
        a5 = np.uint64(0xA5A5A5A5A5A5A5A5)
        if not ((beg.numpy()[first[0]:] == a5).all() and (end.numpy()[first[0]:] == a5).all()):
            raise _lib.WgaError("wga_paf_fix_plan wrote outside its span arrays")
        return first[0], (None if first[1] == int(NONE) else first[1]), beg, end

    def paf_fix(self, text, n_bytes, lines, n_lines, counts, n_records, want=(True, True, True)):
        """K29: the rows with corrected ends and the two invalid lists from wga_cigar_stat's counts of the records, both calls
        of wga_paf_fix.  want = which of (rows, qlist, tlist) the second call is given a buffer for.  Returns (rows, qlist,
        tlist, sizes as a dict), a text that was not asked for as None; the 64 bytes in front of and behind every text are
        checked."""
        n_lines = int(n_lines)
        work = self.empty(max(int(self.lib.wga_paf_fix_work_bytes(n_lines)), 16), np.uint8)
        sizes = np.zeros(1, dtype=PAF_FIX_SIZES_DTYPE)
        args = (self.ctx, _p(text), int(n_bytes), _p(lines), n_lines, _p(counts), int(n_records), _p(work), sizes.ctypes.data)
        self._check(self.lib.wga_paf_fix(*args, None, None, None))
        first = sizes.copy()
        guard = 64  # bytes around each text that the fill call must leave alone
        nbytes = [int(first[k][0]) for k in ("rows_bytes", "qlist_bytes", "tlist_bytes")]
        outs = [self.upload(np.full(nb + 2 * guard, 0xA5, dtype=np.uint8)) if w else None for nb, w in zip(nbytes, want)]
        if any(want):
            self._check(self.lib.wga_paf_fix(*args, *[o.ptr + guard if o is not None else None for o in outs]))
        self.sync()
        if sizes.tobytes() != first.tobytes():
            raise _lib.WgaError("wga_paf_fix changed *sizes in the second call")
        texts = []
        for o, nb in zip(outs, nbytes):
            if o is None:
                texts.append(None)
                continue
            got = o.numpy()
            if not ((got[:guard] == 0xA5).all() and (got[guard + nb:] == 0xA5).all()):
                raise _lib.WgaError("wga_paf_fix wrote outside a text's extent")
            texts.append(got[guard:guard + nb].tobytes())
        return texts[0], texts[1], texts[2], {k: int(first[k][0]) for k in PAF_FIX_SIZES_DTYPE.names}

    def maf_split(self, text, n_bytes, lines=None):
        """K14: number of text lines (lines is None), or the wga_maf_line of every line"""
        nl = C.c_uint64(0)
        cap = 0 if lines is None else (lines.numel() if hasattr(lines, "numel") else lines.size)
        self._check(self.lib.wga_maf_split(self.ctx, _p(text), int(n_bytes), C.byref(nl), _p(lines), int(cap)))
        return int(nl.value)

    def maf_index(self, text, n_bytes, lines, n_lines, skip=0, base=0, carry_offset=0, work=None, out_shift=0):
        """K35 (index.rs:14-94): the blocks' offsets, the name groups and the JSON interval text of a piece, both calls of
        wga_maf_index on wga_maf_split's table.  Returns a dict: n_names, n_blocks, n_slines, first_dup_line and
        first_conflict_line (None when absent), next_offset, names (numpy MAF_INDEX_NAME_DTYPE, n_names + 1 entries) and text —
        or None for a table with a WGA_MAF_FALLBACK line (WGA_E_FALLBACK).  The 64 bytes in front of and behind the text and the
        entry behind the table are checked to be left alone, after the count call and after the fill; the counts must stay.
        work: a device buffer to use; out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n_lines = int(n_lines)
        if work is None:
            work = self.empty(max(int(self.lib.wga_maf_index_work_bytes(n_lines)), 16), np.uint8)
        host = [C.c_uint64(7) for _ in range(7)]
        args = (self.ctx, _p(text), int(n_bytes), _p(lines), n_lines, int(skip), int(base), int(carry_offset), _p(work)) + \
            tuple(C.byref(v) for v in host)
        rc = self.lib.wga_maf_index(*args, None, None)
        if rc == E_FALLBACK:
            return None
        self._check(rc)
        first = [int(v.value) for v in host]
        n_names, n_blocks, n_slines, total, dup, conflict, nxt = first
        guard = 64
        out = self.upload(np.full(total + 2 * guard + 32, 0xA5, dtype=np.uint8))
        names = self.upload(np.full((n_names + 2) * 48, 0xA5, dtype=np.uint8))
        self._check(self.lib.wga_maf_index(*args, names.ptr, out.ptr + guard + int(out_shift)))
        self.sync()
        if [int(v.value) for v in host] != first:
            raise _lib.WgaError("wga_maf_index changed its counts in the second call")
        got, lead = out.numpy(), guard + int(out_shift)
        tab = names.numpy()
        if not ((got[:lead] == 0xA5).all() and (got[lead + total:] == 0xA5).all()):
            raise _lib.WgaError("wga_maf_index wrote outside d_out[0 .. text_bytes)")
        used = (n_names + 1) * 48 if n_slines else 0
        if not (tab[used:] == 0xA5).all():
            raise _lib.WgaError("wga_maf_index wrote behind its table")
        none = int(NONE)
        return dict(n_names=n_names, n_blocks=n_blocks, n_slines=n_slines, next_offset=nxt,
                    first_dup_line=None if dup == none else dup, first_conflict_line=None if conflict == none else conflict,
                    names=tab[:used].view(MAF_INDEX_NAME_DTYPE).copy(), text=got[lead:lead + total].tobytes())

    def chain_split(self, text, n_bytes, heads=None, lines=None, line_off=None):
        """K23: (n_chains, n_data_lines, status, first bad line or None); the count call when the three arrays are None,
        else they are filled (heads: CHAIN_HEAD_DTYPE, lines: n x 3 u64, line_off: n_chains + 1 u64)"""
        nc, nd, st, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)

        def cap(a, per):
            return 0 if a is None else (a.numel() if hasattr(a, "numel") else a.size) // per
        self._check(self.lib.wga_chain_split(self.ctx, _p(text), int(n_bytes), C.byref(nc), C.byref(nd), C.byref(st),
                                             C.byref(bad), _p(heads), cap(heads, 1), _p(lines), cap(lines, 3), _p(line_off)))
        return int(nc.value), int(nd.value), int(st.value), None if bad.value == int(NONE) else int(bad.value)

    def chain_line_off_rebase(self, n, line_off, out=None):
        """K23's offsets of a run of n chains (line_off: its first entry, a device pointer) as a batch of its own: out[i] = line_off[i] - line_off[0]"""
        out = out if out is not None else self.empty(n + 1, np.uint64)
        self._check(self.lib.wga_chain_line_off_rebase(self.ctx, int(n), _p(line_off), _p(out)))
        return out

    def _count_then_fill(self, name, what, args, n_outs, out_shift, types=None, fixed=None):
        """both calls of the text writer `name`: args, then n_outs results by reference (*total_bytes first; u64, or the ctypes
        `types`), then d_out.
        The fill goes into a buffer of 0xA5 and must leave the results (`what` names them; the first `fixed` of them where the
        fill call sets the others) and the bytes around the text alone.
        Returns (text, the results as the fill call leaves them)."""
        fn = getattr(self.lib, name)
        outs = [t(0) for t in (types or [C.c_uint64] * n_outs)]
        refs = [C.byref(o) for o in outs]
        self._check(fn(*args, *refs, None))
        first = tuple(int(o.value) for o in outs)
        guard = 64  # bytes around the text that the fill call must leave alone
        out = self.upload(np.full(first[0] + 2 * guard + 96, 0xA5, dtype=np.uint8))
        lead = guard + (-out.ptr) % 64 + int(out_shift)
        self._check(fn(*args, *refs, out.ptr + lead))
        self.sync()
        last = tuple(int(o.value) for o in outs)
        if last[:fixed] != first[:fixed]:
            raise _lib.WgaError("%s changed its %s in the second call" % (name, what))
        got = out.numpy()
        if not ((got[:lead] == 0xA5).all() and (got[lead + first[0]:] == 0xA5).all()):
            raise _lib.WgaError("%s wrote outside d_out[0 .. total_bytes)" % name)
        return got[lead:lead + first[0]].tobytes(), last

    def chain_filter_count(self, text, n_bytes, heads, n_chains, lines, line_off, work, min_block_size=0, min_query_size=0):
        """K25: the count call of wga_chain_filter alone, (total_bytes, n_kept); it leaves its plan and item scan in `work`"""
        par = np.zeros(1, dtype=CHAIN_FILTER_PARAMS_DTYPE)
        par["min_block_size"], par["min_query_size"] = int(min_block_size), int(min_query_size)
        total, kept = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.wga_chain_filter(self.ctx, _p(text), int(n_bytes), _p(heads), int(n_chains), _p(lines), _p(line_off),
                                              par.ctypes.data, _p(work), C.byref(total), C.byref(kept), None))
        return int(total.value), int(kept.value)

    def chain_filter(self, text, n_bytes, heads, n_chains, lines, line_off, min_block_size=0, min_query_size=0, work=None,
                     n_data_lines=None, out_shift=0):
        """K25 (chain.rs:92-100,185-204 behind filter.rs:91-105): the text of the kept chains of wga_chain_split's arrays, both
        calls of wga_chain_filter.  Returns (text, n_kept); the 64 bytes in front of and behind the text are checked.
        work: a device buffer to use (else one of wga_chain_filter_work_bytes, for which n_data_lines is read from line_off when
        it is not given); out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n_chains = int(n_chains)
        if work is None:
            if n_data_lines is None:
                n_data_lines = int(line_off.numpy()[n_chains]) if n_chains else 0
            work = self.empty(max(int(self.lib.wga_chain_filter_work_bytes(n_chains, int(n_data_lines))), 16), np.uint8)
        par = np.zeros(1, dtype=CHAIN_FILTER_PARAMS_DTYPE)
        par["min_block_size"], par["min_query_size"] = int(min_block_size), int(min_query_size)
        args = (self.ctx, _p(text), int(n_bytes), _p(heads), n_chains, _p(lines), _p(line_off), par.ctypes.data, _p(work))
        text, (_, kept) = self._count_then_fill("wga_chain_filter", "counts", args, 2, out_shift)
        return text, kept

    def chain2paf_count(self, text, n_bytes, heads, n_chains, lines, line_off, work):
        """K27: the count call of wga_chain2paf alone, total_bytes; it leaves its sums, plan and item scan in `work`"""
        total = C.c_uint64(0)
        self._check(self.lib.wga_chain2paf(self.ctx, _p(text), int(n_bytes), _p(heads), int(n_chains), _p(lines), _p(line_off),
                                           _p(work), C.byref(total), None))
        return int(total.value)

    def chain2paf(self, text, n_bytes, heads, n_chains, lines, line_off, work=None, n_data_lines=None, out_shift=0):
        """K27 (chain.rs:430-452 over cigar.rs:554-627): the PAF records of wga_chain_split's arrays, both calls of wga_chain2paf.
        Returns the text; the 64 bytes in front of and behind it are checked.
        work: a device buffer to use (else one of wga_chain2paf_work_bytes, for which n_data_lines is read from line_off when it is
        not given); out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n_chains = int(n_chains)
        if work is None:
            if n_data_lines is None:
                n_data_lines = int(line_off.numpy()[n_chains]) if n_chains else 0
            work = self.empty(max(int(self.lib.wga_chain2paf_work_bytes(n_chains, int(n_data_lines))), 16), np.uint8)
        args = (self.ctx, _p(text), int(n_bytes), _p(heads), n_chains, _p(lines), _p(line_off), _p(work))
        return self._count_then_fill("wga_chain2paf", "total", args, 1, out_shift)[0]

    def maf2paf_count(self, n, names, n_name_bytes, heads, counts, runs, run_off, cols, work):
        """K28: the count call of wga_maf2paf alone, total_bytes; it leaves its sums, plan and item scan in `work`"""
        total = C.c_uint64(0)
        self._check(self.lib.wga_maf2paf(self.ctx, int(n), _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(runs), _p(run_off),
                                         _p(cols), _p(work), C.byref(total), None))
        return int(total.value)

    def maf2paf(self, n, names, n_name_bytes, heads, counts, runs, run_off, cols, work=None, n_runs=None, out_shift=0):
        """K28 (the record of maf.rs:484-520): the PAF records of n blocks from wga_maf_pair_stat's counters and runs and the
        caller's heads (MAF2PAF_HEAD_DTYPE), both calls of wga_maf2paf.  Returns the text; the 64 bytes in front of and behind it
        are checked.
        work: a device buffer to use (else one of wga_maf2paf_work_bytes, for which n_runs is read from run_off when it is not
        given); out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            if n_runs is None:
                n_runs = int(run_off.numpy()[n]) if n else 0
            work = self.empty(max(int(self.lib.wga_maf2paf_work_bytes(n, int(n_runs))), 16), np.uint8)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(runs), _p(run_off), _p(cols), _p(work))
        return self._count_then_fill("wga_maf2paf", "total", args, 1, out_shift)[0]

    def chain_heads_count(self, n, names, n_name_bytes, heads, trim, nbytes, diag, chain_id0, work, data_off):
        """K30: the count call of wga_chain_heads alone, (total_bytes, n_good); it leaves its plan and the records' places in
        `work` and the places of K10's data lines in `data_off`"""
        total, good = C.c_uint64(0), C.c_uint32(0)
        self._check(self.lib.wga_chain_heads(self.ctx, int(n), _p(names), int(n_name_bytes), _p(heads), _p(trim), _p(nbytes), _p(diag),
                                             int(chain_id0), _p(work), _p(data_off), C.byref(total), C.byref(good), None))
        return int(total.value), int(good.value)

    def chain_heads(self, n, names, n_name_bytes, heads, trim, nbytes, diag, chain_id0=0, work=None, data_off=None, out_shift=0):
        """K30 (chain.rs:103-203): the heads and the "\n\n" of n chain records around the places of K10's data lines, both calls
        of wga_chain_heads on wga_cigar_chain's count results and the caller's heads (MAF2PAF_HEAD_DTYPE).  Returns (text, n_good,
        data_off): the fill goes into a buffer of 0xA5, so the data lines' gaps hold that byte; the 64 bytes in front of and behind
        the text are checked.
        work, data_off: device buffers to use; out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_chain_heads_work_bytes(n)), 16), np.uint8)
        if data_off is None:
            data_off = self.empty(max(n, 1), np.uint64)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(trim), _p(nbytes), _p(diag), int(chain_id0), _p(work),
                _p(data_off))
        text, (_, good) = self._count_then_fill("wga_chain_heads", "counts", args, 2, out_shift, types=(C.c_uint64, C.c_uint32))
        return text, good, data_off

    def chain_records(self, batch, names, heads, chain_id0=0, out_shift=0):
        """paf2chain's / maf2chain's records of a batch: K10 count -> K30 count -> K10 fill at K30's places, over the n_good records in
        front of the first bad one -> K30 fill.  names: the bytes the heads' spans point into, heads: MAF2PAF_HEAD_DTYPE (host
        arrays or device arrays).  Returns (text, n_good); the 64 bytes in front of and behind the text are checked."""
        n = batch.n
        if not isinstance(names, DeviceArray):
            names = self.upload(np.frombuffer(bytes(names), dtype=np.uint8)) if len(names) else None
        n_name_bytes = names.size if names is not None else 0
        if not isinstance(heads, DeviceArray):
            heads = self.upload(np.ascontiguousarray(heads, dtype=MAF2PAF_HEAD_DTYPE)) if n else None
        trim, nbytes, diag = self.cigar_chain(batch)
        work = self.empty(max(int(self.lib.wga_chain_heads_work_bytes(n)), 16), np.uint8)
        data_off = self.empty(max(n, 1), np.uint64)
        hargs = (n, names, n_name_bytes, heads, trim, nbytes, diag, chain_id0, work, data_off)
        total, good = self.chain_heads_count(*hargs)
        guard = 64
        out = self.upload(np.full(total + 2 * guard + 96, 0xA5, dtype=np.uint8))
        lead = guard + (-out.ptr) % 64 + int(out_shift)
        if good:
            self.cigar_chain(Batch(batch.ops, batch.op_off, batch.strand_neg, good, batch.n_ops), out=out.ptr + lead, out_off=data_off)
        tb, gd = C.c_uint64(total), C.c_uint32(good)
        self._check(self.lib.wga_chain_heads(self.ctx, n, _p(names), n_name_bytes, _p(heads), _p(trim), _p(nbytes), _p(diag),
                                             int(chain_id0), _p(work), _p(data_off), C.byref(tb), C.byref(gd), out.ptr + lead))
        self.sync()
        got = out.numpy()
        if not ((got[:lead] == 0xA5).all() and (got[lead + total:] == 0xA5).all()):
            raise _lib.WgaError("chain_records wrote outside d_out[0 .. total_bytes)")
        return got[lead:lead + total].tobytes(), good

    def maf_frame_count(self, n, names, n_name_bytes, heads, counts, t_src_len, q_src_len, work, t_row_off, q_row_off, rec_off,
                        diag=None):
        """K32: the count call of wga_paf2maf_frame alone, total_bytes; it leaves the heads' byte counts in `work` and the
        layout in t_row_off[n], q_row_off[n] and rec_off[n + 1]"""
        total, good, gb = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self.lib.wga_paf2maf_frame(self.ctx, int(n), _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(t_src_len),
                                               _p(q_src_len), _p(diag), _p(work), _p(t_row_off), _p(q_row_off), _p(rec_off),
                                               C.byref(total), C.byref(good), C.byref(gb), None))
        return int(total.value)

    def maf_frame(self, n, names, n_name_bytes, heads, counts, t_src_len, q_src_len, diag=None, work=None, out_shift=0):
        """K32 (maf.rs:566-581): the frames of n MAF records around the places of their rows, both calls of wga_paf2maf_frame
        on wga_cigar_stat's counters (or arrays of the same meaning) and the caller's heads (MAF_FRAME_HEAD_DTYPE).  Returns
        (text, n_good, good_bytes, (t_row_off, q_row_off, rec_off)): the fill goes into a buffer of 0xA5, so the rows' places hold
        that byte; the 64 bytes in front of and behind the text are checked.
        work: a device buffer to use; out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_paf2maf_frame_work_bytes(n)), 16), np.uint8)
        lay = (self.empty(max(n, 1), np.uint64), self.empty(max(n, 1), np.uint64), self.empty(n + 1, np.uint64))
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(t_src_len), _p(q_src_len), _p(diag), _p(work),
                _p(lay[0]), _p(lay[1]), _p(lay[2]))
        text, (_, good, gb) = self._count_then_fill("wga_paf2maf_frame", "total", args, 3, out_shift,
                                                    types=(C.c_uint64, C.c_uint32, C.c_uint64), fixed=1)  # the fill finds the bad
        return text, good, gb, lay

    def maf_records(self, batch, names, heads, t_fa, t_fa_bytes, t_src_off, t_src_len, q_fa, q_fa_bytes, q_src_off, q_src_len,
                    out_shift=0):
        """paf2maf's / chain2maf's records of a batch: K1 -> K32 count -> the row kernel at K32's places -> K32 fill.  names: the bytes the heads' spans point into, heads: MAF_FRAME_HEAD_DTYPE (host
        arrays or device arrays); the pools and slices as for paf2maf_expand.  Returns (the text of the records in front of the
        first bad one, n_good, the whole text); the 64 bytes in front of and behind the text are checked."""
        n = batch.n
        if not isinstance(names, DeviceArray):
            names = self.upload(np.frombuffer(bytes(names), dtype=np.uint8)) if len(names) else None
        n_name_bytes = names.size if names is not None else 0
        if not isinstance(heads, DeviceArray):
            heads = self.upload(np.ascontiguousarray(heads, dtype=MAF_FRAME_HEAD_DTYPE)) if n else None
        counts, diag, tile_ws = self.cigar_stat(batch)
        work = self.empty(max(int(self.lib.wga_paf2maf_frame_work_bytes(n)), 16), np.uint8)
        lay = (self.empty(max(n, 1), np.uint64), self.empty(max(n, 1), np.uint64), self.empty(n + 1, np.uint64))
        args = (self.ctx, n, _p(names), n_name_bytes, _p(heads), _p(counts), _p(t_src_len), _p(q_src_len), _p(diag), _p(work),
                _p(lay[0]), _p(lay[1]), _p(lay[2]))
        total, good, gb = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        refs = (C.byref(total), C.byref(good), C.byref(gb))
        self._check(self.lib.wga_paf2maf_frame(*args, *refs, None))
        first = int(total.value)
        guard = 64
        out = self.upload(np.full(first + 2 * guard + 96, 0xA5, dtype=np.uint8))
        lead = guard + (-out.ptr) % 64 + int(out_shift)
        if n:
            self.paf2maf_expand(batch, counts, tile_ws, t_fa, t_fa_bytes, t_src_off, t_src_len, q_fa, q_fa_bytes, q_src_off,
                                q_src_len, out.ptr + lead, lay[0], lay[1], diag)
        self._check(self.lib.wga_paf2maf_frame(*args, *refs, out.ptr + lead))
        self.sync()
        got = out.numpy()
        if int(total.value) != first or not ((got[:lead] == 0xA5).all() and (got[lead + first:] == 0xA5).all()):
            raise _lib.WgaError("maf_records wrote outside d_out[0 .. total_bytes)")
        text = got[lead:lead + first].tobytes()
        return text[:int(gb.value)], int(good.value), text

    def stat_rows_count(self, n, names, n_name_bytes, heads, counts, work, row_off):
        """K33: the count call of wga_stat_rows alone, total_bytes; it leaves the rows' byte counts in `work` and their places in
        row_off[n + 1]"""
        total = C.c_uint64(0)
        self._check(self.lib.wga_stat_rows(self.ctx, int(n), _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(work),
                                           _p(row_off), C.byref(total), None))
        return int(total.value)

    def stat_rows(self, n, names, n_name_bytes, heads, counts, work=None, out_shift=0):
        """K33 (stat.rs:129-164): the TSV rows of `stat --each` for n records, both calls of wga_stat_rows on wga_cigar_stat's or
        wga_maf_pair_stat's counters (or arrays of the same meaning) and the caller's heads (STAT_ROW_HEAD_DTYPE).  Returns
        (text, row_off); the guard bytes in front of and behind the text are checked after the count call and after the fill.
        work: a device buffer to use; out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_stat_rows_work_bytes(n)), 16), np.uint8)
        row_off = self.empty(n + 1, np.uint64)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(work), _p(row_off))
        text = self._count_then_fill("wga_stat_rows", "total", args, 1, out_shift)[0]
        return text, (row_off.numpy().copy() if n else np.zeros(1, np.uint64))

    def _bits_text(self, name, bits, dtype, slot, longest):
        """a formatter alone (wga_f32_text, wga_f64_text): the texts of the values with the bit patterns `bits`, a list of bytes.
        The text buffer, `slot` bytes per value, is filled with 0xA5 first: a text may not reach beyond its length"""
        fn = getattr(self.lib, name)
        bits = np.ascontiguousarray(bits, dtype=dtype)
        n = int(bits.size)
        if n == 0:
            self._check(fn(self.ctx, 0, None, None, None))
            return []
        d_bits = self.upload(bits)
        d_text = self.upload(np.full(slot * n, 0xA5, dtype=np.uint8))
        d_len = self.upload(np.full(n, 0xFF, dtype=np.uint8))
        self._check(fn(self.ctx, n, _p(d_bits), _p(d_text), _p(d_len)))
        self.sync()
        text = d_text.numpy().reshape(n, slot)
        ln = d_len.numpy()
        if (ln > longest).any() or not (text[np.arange(slot)[None, :] >= ln[:, None]] == 0xA5).all():
            raise _lib.WgaError("%s wrote behind a text's length" % name)
        flat = text.tobytes()
        return [flat[slot * i:slot * i + k] for i, k in enumerate(ln.tolist())]

    def f32_text(self, bits):
        """K33's formatter alone: the texts of the f32s with the bit patterns `bits` (uint32)"""
        return self._bits_text("wga_f32_text", bits, np.uint32, 16, 16)

    def stat_pairs(self, n, names, n_name_bytes, heads, counts, inv_in=None, work=None):
        """K36 (stat.rs:167-223): the pairs of n records, both calls of wga_stat_pairs on wga_stat_rows' inputs.  Returns
        (pairs: STAT_PAIR_DTYPE[n_pairs], pair_of_rec: uint32[n]); the words around both outputs are guards and are checked.
        inv_in: a device array of f32 bit patterns, the folds' start values; work: a device buffer to use"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_stat_pairs_work_bytes(n)), 16), np.uint8)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(counts), _p(work))
        n_pairs = C.c_uint64(0)
        self._check(self.lib.wga_stat_pairs(*args, C.byref(n_pairs), None, None, None, 0))
        np_ = int(n_pairs.value)
        guard = 2
        d_pairs = self.upload(np.full((np_ + 2 * guard) * 32, 0xA5A5A5A5, dtype=np.uint32))
        d_por = self.upload(np.full(n + 2 * guard * 32, 0xA5A5A5A5, dtype=np.uint32))
        self._check(self.lib.wga_stat_pairs(*args, C.byref(n_pairs), d_por.ptr + guard * 128, _p(inv_in), d_pairs.ptr + guard * 128,
                                            np_))
        self.sync()
        if int(n_pairs.value) != np_:
            raise _lib.WgaError("wga_stat_pairs changed its n_pairs in the second call")
        gp, gr = d_pairs.numpy(), d_por.numpy()
        lead = guard * 32
        if not ((gp[:lead] == 0xA5A5A5A5).all() and (gp[lead + np_ * 32:] == 0xA5A5A5A5).all() and
                (gr[:lead] == 0xA5A5A5A5).all() and (gr[lead + n:] == 0xA5A5A5A5).all()):
            raise _lib.WgaError("wga_stat_pairs wrote outside d_pairs[0 .. n_pairs) or d_pair_of_rec[0 .. n)")
        return gp[lead:lead + np_ * 32].copy().view(STAT_PAIR_DTYPE), gr[lead:lead + n].copy()

    def stat_pair_rows(self, n, names, n_name_bytes, heads, sums, inv_bits, work=None, out_shift=0):
        """K36 (stat.rs:216-218): the TSV rows of the merged table for n pairs, both calls of wga_stat_pair_rows on the pairs'
        heads (STAT_ROW_HEAD_DTYPE: sizes, minima, names), sums (COUNTS_DTYPE) and inv_size bit patterns (uint32).  Returns
        (text, row_off), checked as stat_rows checks"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_stat_rows_work_bytes(n)), 16), np.uint8)
        row_off = self.empty(n + 1, np.uint64)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(sums), _p(inv_bits), _p(work), _p(row_off))
        text = self._count_then_fill("wga_stat_pair_rows", "total", args, 1, out_shift)[0]
        return text, (row_off.numpy().copy() if n else np.zeros(1, np.uint64))

    def dotplot_overview(self, n, names, n_name_bytes, heads, counts, no_identity=False, work=None, out_shift=0):
        """K34 (dotplot.rs:384-423): the csv rows of `dotplot -m overview` for n records, both calls of wga_dotplot_overview on
        wga_cigar_stat's or wga_maf_pair_stat's counters (or an array of the same meaning; None under no_identity) and the
        caller's heads (DOTPLOT_OV_HEAD_DTYPE).  Returns (text, row_off); the guard bytes in front of and behind the text are
        checked after the count call and after the fill.
        work: a device buffer to use; out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            work = self.empty(max(int(self.lib.wga_dotplot_overview_work_bytes(n)), 16), np.uint8)
        row_off = self.empty(n + 1, np.uint64)
        args = (self.ctx, n, _p(names), int(n_name_bytes), _p(heads), _p(counts), 1 if no_identity else 0, _p(work), _p(row_off))
        text = self._count_then_fill("wga_dotplot_overview", "total", args, 1, out_shift)[0]
        return text, (row_off.numpy().copy() if n else np.zeros(1, np.uint64))

    def f64_text(self, bits):
        """K34's formatter alone: the texts of the f64s with the bit patterns `bits` (uint64)"""
        return self._bits_text("wga_f64_text", bits, np.uint64, 32, 24)

    def pafpseudo_frame(self, items, pool, pool_bytes, text, text_bytes, out, out_bytes, first_bad=None):
        """K31 (the rows of pseudomaf.rs:98-209 around the segments): writes every FILL / COPY span of `items` (SPAN_ITEM_DTYPE, a
        host array or a device array) into out[0, out_bytes) and leaves the holes alone; wga_pafpseudo_frame.  pool / text / out:
        device arrays or pointers (out 16-byte aligned).  Returns the index of the first bad item, or None"""
        if not isinstance(items, DeviceArray):
            items = self.upload(np.ascontiguousarray(items, dtype=SPAN_ITEM_DTYPE))
        first_bad = first_bad if first_bad is not None else self.empty(1, np.uint64)
        self._check(self.lib.wga_pafpseudo_frame(self.ctx, items.size, _p(items), _p(pool), int(pool_bytes), _p(text), int(text_bytes),
                                                 _p(out), int(out_bytes), _p(first_bad)))
        bad = int(first_bad.numpy()[0])
        return None if bad == 0xFFFFFFFFFFFFFFFF else bad

    def dotplot_csv_count(self, n, segs, seg_off, tails, tail_off, work):
        """K26: the count call of wga_dotplot_csv alone, total_bytes; it leaves the scan of the row sizes in `work`"""
        total = C.c_uint64(0)
        self._check(self.lib.wga_dotplot_csv(self.ctx, int(n), _p(segs), _p(seg_off), _p(tails), _p(tail_off), _p(work),
                                             C.byref(total), None))
        return int(total.value)

    def dotplot_csv(self, n, segs, seg_off, tails, tail_off, work=None, n_rows=None, out_shift=0):
        """K26 (the csv rows of dotplot.rs:208-262, base-level): `<s0>,<s1>,<s2>,<s3>,<M|I|D>` and the record's tail for every
        segment of wga_cigar_dotplot's arrays, both calls of wga_dotplot_csv.  Returns the text; the 64 bytes in front of and
        behind it are checked.
        work: a device buffer to use (else one of wga_dotplot_csv_work_bytes, for which n_rows is read from seg_off when it is not
        given); out_shift: d_out starts that many bytes behind a 64-byte aligned address"""
        n = int(n)
        if work is None:
            if n_rows is None:
                n_rows = int(seg_off.numpy()[n]) if n else 0
            work = self.empty(max(int(self.lib.wga_dotplot_csv_work_bytes(int(n_rows))), 16), np.uint8)
        args = (self.ctx, n, _p(segs), _p(seg_off), _p(tails), _p(tail_off), _p(work))
        return self._count_then_fill("wga_dotplot_csv", "total", args, 1, out_shift)[0]

    def cigar_tokenise_spans(self, n, text, beg, end, op_cnt=None, err=None, ops=None, op_off=None):
        """device tokeniser on spans text[beg[i], end[i]) (e.g. the cg:Z: texts inside a PAF file)"""
        op_cnt = op_cnt if op_cnt is not None else self.empty(n, np.uint64)
        err = err if err is not None else self.empty(n, TOK_ERR_DTYPE)
        self._check(self.lib.wga_cigar_tokenise_spans(self.ctx, n, _p(text), _p(beg), _p(end), _p(op_cnt), _p(err),
                                                      _p(ops), _p(op_off)))
        return op_cnt, err

    def counts_total(self, n, counts, totals=None):
        """column sums of the n x 11 counter matrix (stat totals)"""
        totals = totals if totals is not None else self.empty(11, np.uint64)
        self._check(self.lib.wga_counts_total(self.ctx, int(n), _p(counts), _p(totals)))
        return totals

    def fasta_pool(self, text, n_bytes):
        """FASTA text in HBM -> (pool DeviceArray, contig table as numpy FA_CONTIG_DTYPE); two calls of wga_fasta_pool"""
        nc, nb = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.wga_fasta_pool(self.ctx, _p(text), int(n_bytes), C.byref(nc), C.byref(nb), None, None))
        pool = self.empty(max(1, nb.value), np.uint8)
        contigs = self.empty(max(1, nc.value), FA_CONTIG_DTYPE)
        self._check(self.lib.wga_fasta_pool(self.ctx, _p(text), int(n_bytes), C.byref(nc), C.byref(nb), _p(pool), _p(contigs)))
        pool.shape = (nb.value,)
        return pool, contigs.numpy()[: nc.value]

    def paf_call_events(self, batch, svlen, snp, ev_cnt=None, ev=None, ev_off=None):
        ev_cnt = ev_cnt if ev_cnt is not None else self.empty(batch.n, np.uint64)
        self._check(self.lib.wga_paf_call_events(self.ctx, C.byref(batch.c), int(svlen), int(bool(snp)),
                                                 _p(ev_cnt), _p(ev), _p(ev_off)))
        return ev_cnt

    def paf_call_vcf(self, batch, svlen, ev, ev_off, recs, names, t_pool, q_pool, nbytes=None, err=None, out=None,
                     out_off=None):
        """the VCF rows of `call` on PAF (wga_paf_call_vcf, K16) on K7's event list: count pass when out is None (returns
        nbytes, err), fill pass otherwise.  recs: n x VCF_REC_DTYPE"""
        if out is None:
            nbytes = nbytes if nbytes is not None else self.empty(batch.n, np.uint64)
            err = err if err is not None else self.empty(batch.n, VCF_ERR_DTYPE)
        self._check(self.lib.wga_paf_call_vcf(self.ctx, C.byref(batch.c), int(svlen), _p(ev), _p(ev_off), _p(recs), _p(names),
                                              _p(t_pool), _p(q_pool), _p(nbytes) if out is None else None,
                                              _p(err) if out is None else None, _p(out), _p(out_off)))
        return nbytes, err

    def pafcov_accumulate(self, batch, target_id, t_start, cov_off, cov_len, cov, total_cov):
        self._check(self.lib.wga_pafcov_accumulate(self.ctx, C.byref(batch.c), _p(target_id),
                                                   _p(t_start), _p(cov_off), _p(cov_len), _p(cov),
                                                   int(total_cov)))

    def pafcov_accumulate_final(self, batch, target_id, t_start, cov_off, cov_len, n_targets, cov, total_cov):
        """the last batch's marks and the marks -> counts scan in one pass over the array"""
        self._check(self.lib.wga_pafcov_accumulate_final(self.ctx, C.byref(batch.c), _p(target_id), _p(t_start), _p(cov_off),
                                                         _p(cov_len), int(n_targets), _p(cov), int(total_cov)))

    def pafcov_finalize(self, n_targets, cov_off, cov_len, cov):
        self._check(self.lib.wga_pafcov_finalize(self.ctx, n_targets, _p(cov_off), _p(cov_len),
                                                 _p(cov)))

    def pafcov_format(self, name, cov, p0, count, line_off=None, out=None):
        """BED text of pafcov for positions p0 .. p0+count-1 (cov = device pointer of position p0's counter)"""
        line_off = line_off if line_off is not None else self.empty(count + 1, np.uint64)
        self._check(self.lib.wga_pafcov_format(self.ctx, _p(name), int(name.numel() if hasattr(name, 'numel') else name.size), _p(cov), int(p0), int(count),
                                               _p(line_off), _p(out)))
        return line_off

    def maf_chunk(self, text, rows, blocks, chunk_len, carry):
        """K20 (chunk.rs:20-90): the MAF text of one window of chunk records.  text / rows / carry: device arrays (rows of
        MAF_CHUNK_ROW_DTYPE, carry = one u64 per row, advanced by the call); blocks: a host array of MAF_CHUNK_BLOCK_DTYPE.
        Returns the window's text as bytes."""
        blocks = np.ascontiguousarray(blocks, dtype=MAF_CHUNK_BLOCK_DTYPE)
        nb = int(blocks.size)
        n_lines = int(sum(int(b["n_rows"]) * (int(b["k_hi"]) - int(b["k_lo"])) for b in blocks))
        d_blocks = self.upload(blocks) if nb else None
        work = self.empty(int(self.lib.wga_maf_chunk_work_bytes(nb, n_lines)), np.uint8)
        total = C.c_uint64(0)
        args = (self.ctx, _p(text), _p(rows), nb, _p(d_blocks), n_lines, int(chunk_len), _p(carry), _p(work), C.byref(total))
        self._check(self.lib.wga_maf_chunk(*args, None))
        out = self.empty(max(int(total.value), 1), np.uint8)
        self._check(self.lib.wga_maf_chunk(*args, _p(out)))
        self.sync()
        return out.numpy()[:int(total.value)].tobytes()

    def maf_slice(self, text, rows, hits):
        """K21 (mafextra.rs:167-232, maf.rs:223-248): the MAF text of a window of hits.  text / rows: device arrays (rows of
        MAF_SLICE_ROW_DTYPE, all of them get a rank directory); hits: a host array of MAF_SLICE_HIT_DTYPE.  Returns (the text
        of the hits in front of the first hit with a short row, that hit's index or None)."""
        hits = np.ascontiguousarray(hits, dtype=MAF_SLICE_HIT_DTYPE)
        nh = int(hits.size)
        n_lines = int(hits["n_rows"].astype(np.uint64).sum()) if nh else 0
        host_rows = rows.numpy() if nh else np.zeros(0, dtype=MAF_SLICE_ROW_DTYPE)
        nr, n_cols = int(host_rows.size), int(host_rows["seq_len"].sum()) if host_rows.size else 0
        d_hits = self.upload(hits) if nh else None
        work = self.empty(int(self.lib.wga_maf_slice_work_bytes(nh, n_lines, nr, n_cols)), np.uint8)
        total, short = C.c_uint64(0), C.c_uint32(0)
        args = (self.ctx, _p(text), _p(rows), nr, n_cols, nh, _p(d_hits), n_lines, _p(work), C.byref(total), C.byref(short))
        self._check(self.lib.wga_maf_slice(*args, None))
        guard = 64  # bytes around the text that the fill call must leave alone
        out = self.upload(np.full(int(total.value) + 2 * guard, 0xA5, dtype=np.uint8))
        self._check(self.lib.wga_maf_slice(*args, out.ptr + guard))
        self.sync()
        got = out.numpy()
        if not ((got[:guard] == 0xA5).all() and (got[guard + int(total.value):] == 0xA5).all()):
            raise _lib.WgaError("wga_maf_slice wrote outside d_out[0 .. text_bytes)")
        return got[guard:guard + int(total.value)].tobytes(), (None if short.value == 0xFFFFFFFF else int(short.value))

    def maf_rewrite(self, text, rows, blocks, min_block_size=None, min_query_size=None, prefixes=None):
        """K22 (filter.rs:65-105, rename.rs, maf.rs:250-261): the MAF text of a window of blocks.  text / rows: device arrays
        (rows of MAF_SLICE_ROW_DTYPE); blocks: a host array of MAF_REWRITE_BLOCK_DTYPE.  The filter is on when either threshold
        is given (the other one is 0); prefixes: a list of bytes, one per row of every block.  Returns (the text of the kept
        blocks in front of the first bad block, the number of them, that block's index or None)."""
        blocks = np.ascontiguousarray(blocks, dtype=MAF_REWRITE_BLOCK_DTYPE)
        nb = int(blocks.size)
        n_lines = int(blocks["n_rows"].astype(np.uint64).sum()) if nb else 0
        d_blocks = self.upload(blocks) if nb else None
        par = np.zeros(1, dtype=MAF_REWRITE_PARAMS_DTYPE)
        if min_block_size is not None or min_query_size is not None:
            par["filter"] = 1
            par["min_block_size"], par["min_query_size"] = int(min_block_size or 0), int(min_query_size or 0)
        if prefixes:
            off = np.cumsum([0] + [len(p) for p in prefixes]).astype(np.uint32)
            d_ptext = self.upload(np.frombuffer(b"".join(prefixes) + b"\0" * 16, dtype=np.uint8))
            d_poff = self.upload(off)
            par["n_prefix"], par["d_prefix_text"], par["d_prefix_off"] = len(prefixes), d_ptext.ptr, d_poff.ptr
        work = self.empty(int(self.lib.wga_maf_rewrite_work_bytes(nb, n_lines)), np.uint8)
        total, kept, bad = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        args = (self.ctx, _p(text), _p(rows), nb, _p(d_blocks), n_lines, par.ctypes.data, _p(work), C.byref(total), C.byref(kept),
                C.byref(bad))
        self._check(self.lib.wga_maf_rewrite(*args, None))
        guard = 64  # bytes around the text that the fill call must leave alone
        out = self.upload(np.full(int(total.value) + 2 * guard, 0xA5, dtype=np.uint8))
        self._check(self.lib.wga_maf_rewrite(*args, out.ptr + guard))
        self.sync()
        got = out.numpy()
        if not ((got[:guard] == 0xA5).all() and (got[guard + int(total.value):] == 0xA5).all()):
            raise _lib.WgaError("wga_maf_rewrite wrote outside d_out[0 .. text_bytes)")
        return (got[guard:guard + int(total.value)].tobytes(), int(kept.value),
                None if bad.value == 0xFFFFFFFF else int(bad.value))

    def pafpseudo_fill(self, batch, base_mode, q_fa, q_fa_bytes, q_src_off, q_src_len, skip, out,
                       dst_off, diag=None):
        diag = diag if diag is not None else self.empty(batch.n, DIAG_DTYPE)
        self._check(self.lib.wga_pafpseudo_fill(self.ctx, C.byref(batch.c), int(base_mode),
                                                _p(q_fa), int(q_fa_bytes), _p(q_src_off),
                                                _p(q_src_len), _p(skip), _p(out), _p(dst_off),
                                                _p(diag)))
        return diag
