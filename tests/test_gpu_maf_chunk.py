"""`chunk` on a real GPU: the `wgatools` binary over libwgahip.so (K20) and the C-ABI entry, the cases of
test_emu_maf_chunk.py, plus one long block at size."""
import os

import numpy as np
import pytest

from wgatools_amd import build
import maf_chunk_cases as mc
import maf_chunk_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(build.CLI_BIN):
        build.build_cli()
    return build.CLI_BIN


def test_chunk_fixture_l300(cli):
    mc.check_fixture(cli)


def test_chunk_random_files_and_lengths(cli, tmp_path):
    mc.check_random_files(cli, tmp_path, seeds=(11, 12, 13, 14), n_blocks=40, max_cols=3000)


def test_chunk_readers_pieces_windows(cli, tmp_path):
    mc.check_readers_pieces_windows(cli, tmp_path)


def test_chunk_empty_inputs(cli, tmp_path):
    mc.check_empty_inputs(cli, tmp_path)


def test_chunk_argument_and_file_errors(cli, tmp_path):
    mc.check_errors(cli, tmp_path)


def test_chunk_streamed_errors(cli, tmp_path):
    mc.check_stream_errors(cli, tmp_path)


def test_chunk_abi_windows(gpu):
    mc.check_abi_shapes(gpu)


def test_chunk_abi_long_rows(gpu):
    mc.check_abi_long_rows(gpu, cols=300000, L=70000)


def test_chunk_abi_record_ends_at_tile_edge(gpu):
    mc.check_abi_record_ends_at_tile_edge(gpu)


def test_chunk_abi_fields_straddle_tile_edge(gpu):
    mc.check_abi_fields_straddle_tile_edge(gpu)


def test_chunk_abi_many_lines_per_tile(gpu):
    mc.check_abi_many_lines_per_tile(gpu)


def _parse_on_device(t, n_lines, width, name_len):
    """the s-lines of chunk text `t` (a uint8 tensor on the GPU) with the slice widths known: their start and size fields
    (int64) and the slices put together; checks that every s-line has its six tabs, the name length and the line end"""
    import torch
    tabs = torch.nonzero(t == 9).flatten()
    assert tabs.numel() == 6 * n_lines
    tabs = tabs.view(n_lines, 6)
    assert bool((t[tabs[:, 0] - 1] == ord("s")).all())
    assert bool((tabs[:, 1] - tabs[:, 0] - 1 == name_len).all())

    def field(a, b):   # the decimal number between tab positions a and b
        v = torch.zeros(n_lines, dtype=torch.int64, device=t.device)
        p10 = 1
        for d in range(20):
            pos = b - 1 - d
            ok = pos > a
            v += torch.where(ok, (t[pos.clamp(min=0)].to(torch.int64) - 48) * p10, 0)
            p10 *= 10
            if not bool(ok.any()):
                break
        return v
    start, size = field(tabs[:, 1], tabs[:, 2]), field(tabs[:, 2], tabs[:, 3])
    w = width.to(torch.int64)
    assert bool((t[tabs[:, 5] + 1 + w] == 10).all())
    total = int(w.sum())
    base = torch.repeat_interleave(tabs[:, 5] + 1, w)
    within = torch.arange(total, device=t.device) - torch.repeat_interleave(torch.cumsum(w, 0) - w, w)
    return start, size, t[base + within]


def test_chunk_configs2_at_size_in_windows(gpu):
    """configs[2]'s shape made on the device: 2 x 10^6 blocks x 1 500 columns x 2 rows at -l 100, through wga_maf_chunk in
    33 windows that end inside blocks (the rows' carries cross them); every start / size against a cumsum of the rows'
    non-gap bytes at the chunk boundaries, the slices put together against the rows"""
    import ctypes as C
    import torch
    from wgatools_amd.engine import MAF_CHUNK_BLOCK_DTYPE, MAF_CHUNK_ROW_DTYPE
    nb, cols, nr, L, nk = 2_000_000, 1500, 2, 100, 15
    g = torch.Generator(device="cuda").manual_seed(11)
    alphabet = torch.tensor(list(b"ACGT-"), dtype=torch.uint8, device="cuda")
    nrow = nb * nr
    text = torch.zeros(nrow * cols + 64, dtype=torch.uint8, device="cuda")
    text[:nrow * cols] = alphabet[torch.randint(0, 5, (nrow * cols,), device="cuda", generator=g)]
    rows = np.zeros(nrow, dtype=MAF_CHUNK_ROW_DTYPE)
    rows["seq_off"] = np.arange(nrow, dtype=np.uint64) * cols
    rows["seq_len"] = cols
    rows["name_len"] = 8
    rows["start"] = np.arange(nrow, dtype=np.uint64) * 1000
    rows["src_size"] = 10 ** 9
    d_rows = gpu.upload(rows)
    carry = gpu.empty(nrow, np.uint64).fill(0)
    grid = text[:nrow * cols].view(nrow, cols)
    cum = torch.cumsum(grid != ord("-"), 1, dtype=torch.int32)
    cum = torch.cat([torch.zeros(nrow, 1, dtype=torch.int32, device="cuda"), cum], 1)
    bnd = torch.arange(0, cols + 1, L, device="cuda")
    sizes = (cum[:, bnd[1:]] - cum[:, bnd[:-1]]).to(torch.int64)                              # [row, chunk]
    starts = torch.arange(nrow, device="cuda", dtype=torch.int64)[:, None] * 1000 + cum[:, bnd[:-1]]
    order = lambda x: x.view(nb, nr, nk).permute(0, 2, 1).reshape(-1)       # line order: block, chunk, row
    exp_size, exp_start = order(sizes), order(starts)
    exp_slices = grid.view(nb, nr, nk, L).permute(0, 2, 1, 3).reshape(-1)
    del cum, sizes, starts
    torch.cuda.synchronize()     # the rows are made on torch's stream; the library launches on a stream of its own
    n_rec = nb * nk
    cuts = [n_rec * i // 33 for i in range(34)]
    assert any(c % nk for c in cuts[1:-1])
    total_lines = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        win = []
        for blk in range(a // nk, (b - 1) // nk + 1):
            win.append((blk * nr, max(a - blk * nk, 0), min(b - blk * nk, nk), nr, 0))
        win = np.array(win, dtype=MAF_CHUNK_BLOCK_DTYPE)
        n_lines = (b - a) * nr
        d_blocks = gpu.upload(win)
        work = gpu.empty(int(gpu.lib.wga_maf_chunk_work_bytes(len(win), n_lines)), np.uint8)
        tb = C.c_uint64(0)
        args = (gpu.ctx, text.data_ptr(), d_rows.ptr, len(win), d_blocks.ptr, n_lines, L, carry.ptr, work.ptr, C.byref(tb))
        gpu._check(gpu.lib.wga_maf_chunk(*args, None))
        out = torch.zeros(int(tb.value) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize() # ... and so is the zero fill: it must not land on the text behind the fill call
        gpu._check(gpu.lib.wga_maf_chunk(*args, out.data_ptr()))
        gpu.sync()
        t = out[:int(tb.value)]
        lo, hi = a * nr, b * nr
        start, size, sl = _parse_on_device(t, n_lines, torch.full((n_lines,), L, device="cuda"), 8)
        assert torch.equal(size, exp_size[lo:hi]), (a, b)
        assert torch.equal(start, exp_start[lo:hi]), (a, b)
        assert torch.equal(sl, exp_slices[lo * L:hi * L]), (a, b)
        assert int((t == 10).sum()) == n_lines + 2 * (b - a)                   # s-lines, "a score" lines, empty lines
        assert bytes(t[:12].cpu().numpy()) == b"a score=255\n"
        total_lines += n_lines
        del out, t, work
    assert total_lines == nb * nk * nr


def test_chunk_one_long_block_at_size(cli, tmp_path):
    """one block of 10^8 columns x 2 rows through the command line at the default window budget: -l 1000000, and -l 7 (about
    1.3 GB of text: several windows, the rows' carries crossing them); every start / size against a cumsum of the rows'
    non-gap bytes at the chunk boundaries, the slices put together against the rows (the output parsed on the device)"""
    import torch
    cols, nr = 10 ** 8, 2
    g = torch.Generator(device="cuda").manual_seed(5)
    alphabet = torch.tensor(list(b"ACGT-"), dtype=torch.uint8, device="cuda")
    rows = alphabet[torch.randint(0, 5, (nr, cols), device="cuda", generator=g)]
    path = str(tmp_path / "long.maf")
    with open(path, "wb") as f:
        f.write(b"##maf version=1\na score=0\n")
        for r in range(nr):
            f.write(b"s c%d %d %d + 999999999 " % (r, 1000 + r, cols) + rows[r].cpu().numpy().tobytes() + b"\n")
    cum = torch.cat([torch.zeros(nr, 1, dtype=torch.int64, device="cuda"),
                     torch.cumsum(rows != ord("-"), 1, dtype=torch.int64)], 1)
    for L in (1000000, 7):
        out_path = str(tmp_path / "o.maf")
        rc, _, err = mc.run(cli, "-r", "-o", out_path, "chunk", path, "-l", str(L))
        assert rc == 0, err
        data = np.fromfile(out_path, dtype=np.uint8)
        os.remove(out_path)
        hdr = ref.header(L)
        assert data[:len(hdr)].tobytes() == hdr
        t = torch.from_numpy(data[len(hdr):]).cuda()
        del data
        bnd = torch.tensor([c for c, _ in ref.chunk_bounds(cols, L)] + [cols], device="cuda")
        nk = bnd.numel() - 1
        width = (bnd[1:] - bnd[:-1]).repeat_interleave(nr)
        start, size, sl = _parse_on_device(t, nk * nr, width, 2)
        exp_size = (cum[:, bnd[1:]] - cum[:, bnd[:-1]]).t().reshape(-1)
        exp_start = (torch.tensor([1000, 1001], device="cuda")[:, None] + cum[:, bnd[:-1]]).t().reshape(-1)
        assert torch.equal(size, exp_size)
        assert torch.equal(start, exp_start)
        # slices in line order: chunk k of row 0, chunk k of row 1, ...
        idx = torch.repeat_interleave(torch.arange(nk * nr, device="cuda"), width)
        row_of = idx % nr
        for r in range(nr):
            assert torch.equal(sl[row_of == r], rows[r])
        del t, sl, idx, row_of
