"""Host-side mirror of the reference's aligner surface for the convex-gap hot path.

``ConvexAlignHip`` plays the role of ``Convex::ConvexAlignFast`` behind ngmlr's
``IAlignment`` interface (reference src/IAlignment.h:211-247): constructed with the
same six scoring floats (src/AlignmentBuffer.h:345-363), ``single_align`` has the
argument meaning and error behaviour of the corridor ``SingleAlign`` overload
(returns -1 and Score -1.0 for "no valid alignment"), and ``batch_align`` is the
``BatchAlign`` slot the reference leaves unimplemented (src/ConvexAlignFast.cpp:441-450).
All compute goes through the C ABI of include/cvx_align.h; the C++ twin of this class
(the actual drop-in) is ngmlr_amd/csrc/convex_align_hip.{h,cpp}.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import capi

DEFAULT_SCORING = dict(match=2.0, mismatch=-5.0, gap_open=-5.0, gap_extend=-5.0,
                       gap_extend_min=-1.0, gap_decay=0.15)  # src/IConfig.h:50-55


class ConvexAlignHip:
    def __init__(self, device: int = 0, max_matrix_mb: int = 10000, lib_path: str = None, scalar_twin: bool = False,
                 nm_regions: bool = False, job_text: bool = False, inv_checks: bool = False, **scoring):
        """scalar_twin: the handle reproduces Convex::ConvexAlign (ngmlr --nosse) instead of Convex::ConvexAlignFast
        (CVX_CREATE_SCALAR_TWIN, include/cvx_align.h); the host text helpers of its batches follow.
        nm_regions: every job delivers the low-identity regions of its tiles with its results (CVX_CREATE_NM_REGIONS,
        Job.regions).
        job_text: every job delivers the device text stage's records and strings with its results (CVX_CREATE_JOB_TEXT, Job.texts).
        inv_checks: every job submitted with a genome delivers the inversion check of each of its regions with them
        (CVX_CREATE_INV_CHECKS, Job.checks); needs nm_regions."""
        self.lib = capi.load(lib_path)
        self.scalar_twin = bool(scalar_twin)
        self.nm_regions = bool(nm_regions)
        self.job_text = bool(job_text)
        self.inv_checks_on = bool(inv_checks)
        sc = dict(DEFAULT_SCORING)
        sc.update(scoring)
        self.params = capi.CvxParams(sc["match"], sc["mismatch"], sc["gap_open"], sc["gap_extend"],
                                     sc["gap_extend_min"], sc["gap_decay"])
        self.h = C.c_void_p()
        flags = (capi.CREATE_SCALAR_TWIN if self.scalar_twin else 0) | (capi.CREATE_NM_REGIONS if self.nm_regions else 0)
        flags |= capi.CREATE_JOB_TEXT if self.job_text else 0
        flags |= capi.CREATE_INV_CHECKS if self.inv_checks_on else 0
        if flags:
            capi.check(self.lib.cvx_create_ex(device, C.byref(self.params), max_matrix_mb, flags, C.byref(self.h)))
        else:
            capi.check(self.lib.cvx_create(device, C.byref(self.params), max_matrix_mb, C.byref(self.h)))

    def stage_kernel_ms(self, stage: int) -> float:
        """cvx_stage_kernel_ms: device time (HIP events) of the kernels of the handle's last call of a next-row stage
        (capi.STAGE_SCORE / STAGE_DECODE / STAGE_SEARCH)."""
        ms = C.c_float()
        capi.check(self.lib.cvx_stage_kernel_ms(self.h, stage, C.byref(ms)))
        return float(ms.value)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.cvx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # IAlignment::GetAlignBatchSize(): the reference's convex aligner answers 0
    # ("no batching"); this backend takes any batch.
    def get_align_batch_size(self) -> int:
        return 1 << 20

    # ------------------------------------------------------------------ staged API
    def _pack(self, tiles: Sequence, closed_form: bool = False):
        """cvx_tile[] for per-tile objects.  closed_form: tiles that carry a corridor descriptor (Tile.desc) hand
        over that instead of their row arrays."""
        n = len(tiles)
        arr = (capi.CvxTile * max(n, 1))()
        keep = []
        for i, t in enumerate(tiles):
            arr[i].ref = t.ref
            arr[i].qry = t.qry
            arr[i].ref_len = len(t.ref)
            arr[i].qry_len = len(t.qry)
            desc = getattr(t, "desc", None) if closed_form else None
            if desc is not None:
                (arr[i].corridor_kind, arr[i].corridor_k, arr[i].corridor_d, arr[i].corridor_right,
                 arr[i].corridor_offset, arr[i].corridor_width) = desc
                keep.append((t.ref, t.qry))
                continue
            off = np.ascontiguousarray(t.row_offset, dtype=np.int32)
            ln = np.ascontiguousarray(t.row_length, dtype=np.int32)
            keep.append((off, ln, t.ref, t.qry))
            arr[i].row_offset = off.ctypes.data
            arr[i].row_length = ln.ctypes.data
            arr[i].row_stride_bytes = 4
        return arr, keep

    def corridor_rows(self, tile):
        """cvx_corridor_rows: the (offset, length) rows the DEVICE derives from the tile's closed form."""
        arr, keep = self._pack([tile], closed_form=True)
        H = len(tile.qry)
        off = np.zeros(max(H, 1), dtype=np.int32)
        ln = np.zeros(max(H, 1), dtype=np.int32)
        capi.check(self.lib.cvx_corridor_rows(self.h, arr, off.ctypes.data, ln.ctypes.data))
        return off[:H], ln[:H]

    def upload(self, tiles: Sequence, closed_form: bool = False) -> "DeviceBatch":
        arr, keep = self._pack(tiles, closed_form)
        b = C.c_void_p()
        capi.check(self.lib.cvx_batch_upload(self.h, len(tiles), arr, C.byref(b)))
        return DeviceBatch(self, b, list(tiles))

    def timed_host_path(self, tiles: Sequence) -> dict:
        """Host buffers in, results out: what cvx_align_batch does, with the stages timed
        separately (seconds of the C calls only; ctypes packing of the tile table excluded)."""
        import time
        arr, keep = self._pack(tiles)
        b = C.c_void_p()
        t0 = time.perf_counter()
        capi.check(self.lib.cvx_batch_upload(self.h, len(tiles), arr, C.byref(b)))
        t1 = time.perf_counter()
        batch = DeviceBatch(self, b, list(tiles))
        try:
            batch.run()
            t2 = time.perf_counter()
            batch.download()
            t3 = time.perf_counter()
        finally:
            batch.free()
        t4 = time.perf_counter()
        return {"upload_s": t1 - t0, "run_s": t2 - t1, "download_s": t3 - t2, "free_s": t4 - t3, "total_s": t4 - t0}

    # ------------------------------------------------------------------ streaming API
    def submit(self, tiles) -> "Job":
        """cvx_submit: host buffers in, nothing waits.  `tiles`: a synth.TileSet (its table points
        into the flat arrays) or a sequence of Tile objects."""
        if hasattr(tiles, "table"):
            tab = tiles.table()
            arr = tab.ctypes.data_as(C.POINTER(capi.CvxTile))
            keep = (tiles, tab)
            n = len(tab)
        else:
            arr, keep = self._pack(tiles)
            n = len(tiles)
        j = C.c_void_p()
        capi.check(self.lib.cvx_submit(self.h, n, arr, C.byref(j)))
        return Job(self, j, n, keep)

    def submit_segments(self, tiles: Sequence, reads, segments, genome: "Genome" = None, ref_positions=None) -> "Job":
        """cvx_submit_segments: cvx_submit (or, with `genome` and `ref_positions`, cvx_submit_windows) with every tile's query
        named as a segment of a read block and written on the device.  tiles: Tile objects; of tile.qry only the length is
        used (the table handed to the library carries NULL query pointers).  reads: a sequence of bytes, or (arena, offsets) as
        KmerIndex.make_arena returns them.  segments: (read, start, flags) per tile, or a SEGMENT_DTYPE array."""
        arr, keep = self._pack(tiles)
        for i in range(len(tiles)):
            arr[i].qry = None
        arena, offsets, n_reads = _window_reads(reads)
        seg = _segments(segments)
        assert len(seg) == len(tiles), "one segment per tile"
        pos = np.ascontiguousarray(ref_positions, dtype=np.uint64) if genome is not None else None
        j = C.c_void_p()
        capi.check(self.lib.cvx_submit_segments(self.h, genome.g if genome is not None else None, len(tiles), arr,
                                                pos.ctypes.data if pos is not None else None, n_reads, arena.ctypes.data, offsets.ctypes.data,
                                                seg.ctypes.data, C.byref(j)))
        return Job(self, j, len(tiles), (keep, arena, offsets, seg, pos))

    def submit_ladder(self, tiles: Sequence, ladders, genome: "Genome" = None, ref_positions=None) -> "Job":
        """cvx_submit_ladder: cvx_submit (or, with `genome` and `ref_positions`, cvx_submit_windows) whose tiles carry the retry
        ladder of AlignmentBuffer::computeAlignment instead of one corridor; the library climbs it on the device.  tiles: Tile
        objects (their corridors are ignored).  ladders: (corridor, left, right, flags) per tile, or a LADDER_DTYPE array."""
        arr, keep = self._pack(tiles, closed_form=True)
        lad = _ladders(ladders)
        assert len(lad) == len(tiles), "one ladder per tile"
        pos = np.ascontiguousarray(ref_positions, dtype=np.uint64) if genome is not None else None
        j = C.c_void_p()
        capi.check(self.lib.cvx_submit_ladder(self.h, genome.g if genome is not None else None, len(tiles), arr,
                                              pos.ctypes.data if pos is not None else None, lad.ctypes.data, C.byref(j)))
        return Job(self, j, len(tiles), (keep, lad, pos))

    def submit_ladder_ex(self, tiles: Sequence, ladders, genome: "Genome" = None, ref_positions=None, reads=None, segments=None) -> "Job":
        """cvx_submit_ladder_ex: submit_ladder on any handle but a service one -- on a ConvexAlignHip(nm_regions / inv_checks /
        job_text) handle Job.regions(), .checks(), .texts() and .texts_raw() answer for the ladder job as for any job, per tile
        from the rung Job.ladder() reports.  reads / segments (both or neither): the queries as segments of a read block, as
        submit_segments takes them; of tile.qry only the length is used then."""
        assert (reads is None) == (segments is None), "reads and segments come together"
        arr, keep = self._pack(tiles, closed_form=True)
        lad = _ladders(ladders)
        assert len(lad) == len(tiles), "one ladder per tile"
        pos = np.ascontiguousarray(ref_positions, dtype=np.uint64) if genome is not None else None
        arena = offsets = seg = None
        n_reads = 0
        if segments is not None:
            for i in range(len(tiles)):
                arr[i].qry = None
            arena, offsets, n_reads = _window_reads(reads)
            seg = _segments(segments)
            assert len(seg) == len(tiles), "one segment per tile"
        j = C.c_void_p()
        capi.check(self.lib.cvx_submit_ladder_ex(self.h, genome.g if genome is not None else None, len(tiles), arr,
                                                 pos.ctypes.data if pos is not None else None, lad.ctypes.data, n_reads,
                                                 arena.ctypes.data if arena is not None else None, offsets.ctypes.data if offsets is not None else None,
                                                 seg.ctypes.data if seg is not None else None, C.byref(j)))
        return Job(self, j, len(tiles), (keep, lad, pos, arena, offsets, seg))

    def stage_segments(self, reads, segments, lengths) -> List[bytes]:
        """cvx_stage_segments: the strings stage_segments_kernel builds for (read, start, flags) + length, back on the host."""
        arena, offsets, n_reads = _window_reads(reads)
        seg = _segments(segments)
        return _stage_segments(lambda *io: self.lib.cvx_stage_segments(self.h, n_reads, arena.ctypes.data, offsets.ctypes.data, len(seg), seg.ctypes.data, *io), lengths)

    def nm_regions_ops(self, results, ops_arena, want_regions: bool = True):
        """cvx_nm_regions_ops: the low-identity regions of op lists the caller holds (a capi.CvxResult array or sequence, and
        the uint32 ops arena its ops_begin / n_ops point into), found on the device.
        -> (offsets uint64[n + 1], regions int32[r, 4] or None when want_regions is False, open records NM_OPEN_DTYPE[n])"""
        n = len(results)
        res = results if isinstance(results, C.Array) else (capi.CvxResult * max(n, 1))(*results)
        arena = np.ascontiguousarray(ops_arena, dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        opn = np.zeros(n, dtype=NM_OPEN_DTYPE)
        lib = self.lib
        capi.check(lib.cvx_nm_regions_ops(self.h, n, res, arena.ctypes.data, len(arena), off.ctypes.data, None, 0, opn.ctypes.data))
        if not want_regions:
            return off, None, opn
        reg = np.zeros((int(off[n]), 4), dtype=np.int32)
        capi.check(lib.cvx_nm_regions_ops(self.h, n, res, arena.ctypes.data, len(arena), off.ctypes.data, reg.ctypes.data, len(reg), opn.ctypes.data))
        return off, reg, opn

    def inv_checks(self, genome: "Genome", qrys: Sequence[bytes], ref_positions, position_offsets, region_off, regions):
        """cvx_inv_checks: checkForSV's two scores for regions the caller holds, scored on the device against the resident genome
        (the kernel a ConvexAlignHip(inv_checks=True) job runs behind its regions finder).  qrys: the tiles' reads;
        ref_positions / position_offsets per tile; region_off uint64[n + 1] and regions int32[r, 4] as Job.regions() returns them.
        -> (checks INV_CHECK_DTYPE[r], the kernel's ms)"""
        call, chk = _inv_checks_call(qrys, ref_positions, position_offsets, region_off, regions)
        ms = C.c_double()
        capi.check(call(lambda *io: self.lib.cvx_inv_checks(self.h, genome.g, *io, C.byref(ms))))
        return chk, float(ms.value)

    # ------------------------------------------------------------------ reference-shaped API
    def batch_align(self, tiles: Sequence, want_nm: bool = True, closed_form: bool = False) -> List[dict]:
        """N x SingleAlign: returns one Align-like dict per tile (keys = the Align fields)."""
        batch = self.upload(tiles, closed_form)
        try:
            batch.run()
            return batch.alignments(want_nm=want_nm)
        finally:
            batch.free()

    def single_align(self, tile, want_nm: bool = True) -> dict:
        return self.batch_align([tile], want_nm=want_nm)[0]


RESULT_DTYPE = np.dtype([("score", np.float32), ("status", np.int32), ("best_ref_index", np.int32),
                         ("best_read_index", np.int32), ("ref_position", np.int32), ("qstart", np.int32),
                         ("qend", np.int32), ("n_ops", np.int32), ("ops_begin", np.uint64), ("cells", np.uint64)])
assert RESULT_DTYPE.itemsize == C.sizeof(capi.CvxResult)
# cvx_nm_open: the state detectMisalignment's peak finder ends in; a region is (ref_start, ref_stop, read_start, read_stop)
NM_OPEN_DTYPE = np.dtype([("open", np.int32), ("distance", np.int32), ("region", np.int32, (4,))])
assert NM_OPEN_DTYPE.itemsize == C.sizeof(capi.CvxNmOpen)


# cvx_inv_check: checkForSV's two scores for one region, capi.CHECK_* in status
INV_CHECK_DTYPE = np.dtype([("score_fwd", np.float32), ("score_rev", np.float32), ("status", np.int32), ("window_chars", np.int32)])
assert INV_CHECK_DTYPE.itemsize == C.sizeof(capi.CvxInvCheck)


# cvx_ladder / cvx_ladder_result
LADDER_DTYPE = np.dtype([("corridor", np.int32), ("left", np.float32), ("right", np.float32), ("flags", np.int32)])
LADDER_RESULT_DTYPE = np.dtype([("rung", np.int32), ("attempts", np.int32), ("width", np.int32), ("reserved", np.int32)])
assert LADDER_DTYPE.itemsize == C.sizeof(capi.CvxLadder) and LADDER_RESULT_DTYPE.itemsize == C.sizeof(capi.CvxLadderResult)


def _ladders(ladders) -> np.ndarray:
    if isinstance(ladders, np.ndarray) and ladders.dtype == LADDER_DTYPE:
        return np.ascontiguousarray(ladders)
    out = np.zeros(len(ladders), dtype=LADDER_DTYPE)
    for i, l in enumerate(ladders):
        out[i] = (int(l[0]), float(l[1]), float(l[2]), int(l[3]))
    return out


def ladder_rung(tile, ladder, m: int):
    """cvx_ladder_rung: rung m of the retry ladder of `tile` (only its two lengths are read); ladder = (corridor, left, right,
    flags).  -> (kind, k, d, right, offset, width), or None where the rung does not exist."""
    return capi.ladder_rung(len(tile.ref), len(tile.qry), ladder, m)


def _inv_checks_call(qrys, ref_positions, position_offsets, region_off, regions):
    """the tile and region arguments both stand-alone check entries take -> (call(entry) -> rc, the records' array)"""
    n = len(qrys)
    arr = (C.c_char_p * max(n, 1))(*[bytes(q) for q in qrys])
    ql = np.array([len(q) for q in qrys], dtype=np.int32)
    pos = np.ascontiguousarray(ref_positions, dtype=np.uint64)
    po = np.ascontiguousarray(position_offsets, dtype=np.int32)
    off = np.ascontiguousarray(region_off, dtype=np.uint64)
    reg = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1, 4)
    assert len(pos) == n and len(po) == n and len(off) == n + 1 and int(off[n]) == len(reg), "one position and offset per tile, region_off[n] regions"
    chk = np.zeros(len(reg), dtype=INV_CHECK_DTYPE)

    def call(entry):
        return entry(n, arr, ql.ctypes.data, pos.ctypes.data, po.ctypes.data, off.ctypes.data, reg.ctypes.data, chk.ctypes.data)
    return call, chk


def inv_checks_host(binref, nibbles, starts, qrys, ref_positions, position_offsets, region_off, regions, lib=None):
    """cvx_inv_checks_host: the same records from an encoded genome on the host (no device): the window decoded statement by
    statement, the scorer's full recurrence.  -> checks INV_CHECK_DTYPE[r]"""
    lib = lib or capi.load()
    b = np.ascontiguousarray(binref, dtype=np.uint8)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    call, chk = _inv_checks_call(qrys, ref_positions, position_offsets, region_off, regions)
    capi.check(call(lambda *io: lib.cvx_inv_checks_host(b.ctypes.data, int(nibbles), st.ctypes.data, len(st), *io)))
    return chk


def nm_regions_host(triples, scan_len: int, lib=None):
    """cvx_nm_regions_host: the peak finder at the top of detectMisalignment over a profile on the host (no device).
    triples: int32[entries, 3] (refPosition, readPosition, nm); scan_len: alignmentLength (rows past the entries are zeros).
    -> (regions int32[r, 4], open record NM_OPEN_DTYPE scalar)"""
    lib = lib or capi.load()
    tri = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
    n = C.c_int64()
    opn = np.zeros(1, dtype=NM_OPEN_DTYPE)
    capi.check(lib.cvx_nm_regions_host(tri.ctypes.data, len(tri), int(scan_len), None, 0, C.byref(n), opn.ctypes.data))
    reg = np.zeros((int(n.value), 4), dtype=np.int32)
    if n.value:
        capi.check(lib.cvx_nm_regions_host(tri.ctypes.data, len(tri), int(scan_len), reg.ctypes.data, len(reg), C.byref(n), opn.ctypes.data))
    return reg, opn[0]


def reclip(rec, cigar: bytes, ext_qstart: int, ext_qend: int, cigar_cap: Optional[int] = None, lib=None):
    """cvx_text_reclip (host code, no device): a record (capi.CvxAlignmentText) and a CIGAR formatted with both external clips zero
    -> (record, CIGAR bytes) as the host text stage returns them with these clips.  cigar_cap: the capacity of the output buffer
    (None: room for everything); the record's cigar_len is the full length whatever fits."""
    lib = lib or capi.load()
    cap = len(cigar) + 32 if cigar_cap is None else int(cigar_cap)
    buf = C.create_string_buffer(max(cap, 1))
    out = capi.CvxAlignmentText()
    capi.check(lib.cvx_text_reclip(C.byref(rec), bytes(cigar), int(ext_qstart), int(ext_qend), buf if cap > 0 else None, cap, C.byref(out)))
    return out, (buf.value if cap > 0 else b"")


class Job:
    """One batch travelling through the streaming form (cvx_submit / cvx_wait / cvx_job_release)."""

    def __init__(self, aligner: "ConvexAlignHip", handle, n: int, keep):
        self.al, self.j, self.n, self._keep = aligner, handle, n, keep
        self.results = None
        self.ops = None

    def wait(self):
        """Blocks until the job is done.  Returns (results, ops): numpy views of the job's pinned
        result records (RESULT_DTYPE) and dense ops arena, valid until release()."""
        res = C.POINTER(capi.CvxResult)()
        ops = C.POINTER(C.c_uint32)()
        n_ops = C.c_uint64()
        capi.check(self.al.lib.cvx_wait(self.al.h, self.j, C.byref(res), C.byref(ops), C.byref(n_ops)))
        self.res_ptr = res
        self.results = (np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint8)), shape=(self.n * RESULT_DTYPE.itemsize,))
                        .view(RESULT_DTYPE) if self.n else np.zeros(0, RESULT_DTYPE))
        self.ops = (np.ctypeslib.as_array(ops, shape=(int(n_ops.value),)) if n_ops.value else np.zeros(0, np.uint32))
        return self.results, self.ops

    def ladder(self) -> np.ndarray:
        """cvx_job_ladder (after wait, a job of submit_ladder): per tile the rung reported (1-based), the attempts made and that
        rung's corridor width, LADDER_RESULT_DTYPE."""
        p = C.c_void_p()
        capi.check(self.al.lib.cvx_job_ladder(self.al.h, self.j, C.byref(p)))
        if not self.n:
            return np.zeros(0, LADDER_RESULT_DTYPE)
        buf = (C.c_uint8 * (self.n * LADDER_RESULT_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=LADDER_RESULT_DTYPE).copy()

    def ladder_info(self) -> dict:
        """cvx_job_ladder_info: rungs the job ran, tiles per rung, sequence bytes moved after the submit call"""
        info = capi.CvxLadderInfo()
        capi.check(self.al.lib.cvx_job_ladder_info(self.j, C.byref(info)))
        return {"rungs_run": int(info.rungs_run), "tiles": [int(x) for x in info.tiles], "seq_bytes_after_submit": int(info.seq_bytes_after_submit)}

    def zero_copy_bytes(self) -> int:
        """cvx_job_zero_copy_bytes: bytes of this job's upload the device pulled straight out of the caller's page-locked memory"""
        n = C.c_uint64()
        capi.check(self.al.lib.cvx_job_zero_copy_bytes(self.j, C.byref(n)))
        return int(n.value)

    def timing(self) -> capi.CvxTiming:
        t = capi.CvxTiming()
        capi.check(self.al.lib.cvx_job_timing(self.j, C.byref(t)))
        return t

    def launches(self) -> list:
        t = self.timing()
        out = []
        for i in range(t.n_fill_launches):
            li = capi.CvxLaunchInfo()
            capi.check(self.al.lib.cvx_job_launch_info(self.j, i, C.byref(li)))
            out.append({k: getattr(li, k) for k, _ in capi.CvxLaunchInfo._fields_})
        return out

    def text_raw(self, ext_qstart=None, ext_qend=None):
        """cvx_job_text: the device-side text stage of every tile of this finished job.
        -> (cvx_alignment_text array, text offsets uint64[n], text bytes)"""
        n = self.n
        out = (capi.CvxAlignmentText * max(n, 1))()
        off = np.zeros(max(n, 1), dtype=np.uint64)
        text = C.c_char_p()
        nbytes = C.c_uint64()
        eq = np.ascontiguousarray(ext_qstart, dtype=np.int32) if ext_qstart is not None else None
        ee = np.ascontiguousarray(ext_qend, dtype=np.int32) if ext_qend is not None else None
        lib = self.al.lib
        lib.cvx_job_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.CvxAlignmentText),
                                     C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        tp = C.c_void_p()
        capi.check(lib.cvx_job_text(self.al.h, self.j, eq.ctypes.data if eq is not None else None,
                                    ee.ctypes.data if ee is not None else None, out, off.ctypes.data,
                                    C.byref(tp), C.byref(nbytes)))
        buf = (C.c_char * int(nbytes.value)).from_address(tp.value) if nbytes.value else None
        return out, off, buf

    def text(self, ext_qstart=None, ext_qend=None) -> List[dict]:
        """-> one dict per tile with the cvx_alignment_text fields + 'cigar' / 'md' (device-side text stage)."""
        out, off, buf = self.text_raw(ext_qstart, ext_qend)
        raw = buf.raw if buf is not None else b""
        res = []
        for i in range(self.n):
            t = out[i]
            d = {f: getattr(t, f) for f, _ in capi.CvxAlignmentText._fields_}
            d["score_bits"] = int(np.float32(t.score).view(np.uint32))
            o = int(off[i])
            d["cigar"] = raw[o:o + t.cigar_len].decode()
            d["md"] = raw[o + t.cigar_len + 1:o + t.cigar_len + 1 + t.md_len].decode()
            res.append(d)
        return res

    def nm_profile(self, first: int = 0, count: Optional[int] = None, to_host: bool = True):
        """cvx_job_nm_profile (after text()/text_raw()): nmPerPosition of the tiles [first, first + count) from the device.
        -> (entry offsets uint64[count + 1], triples int32[entries, 3] or None when to_host is False, kernel ms)"""
        count = self.n - first if count is None else count
        off = np.zeros(count + 1, dtype=np.uint64)
        ms = C.c_double()
        lib = self.al.lib
        if not to_host:      # the profile stays in HBM (a NULL buffer), for a consumer on the device
            capi.check(lib.cvx_job_nm_profile(self.al.h, self.j, first, count, off.ctypes.data, None, 0, C.byref(ms)))
            return off, None, ms.value
        # sizes first (the offsets alone: no profile kernel, no arena), then the one real call
        capi.check(lib.cvx_job_nm_sizes(self.al.h, self.j, first, count, off.ctypes.data))
        tri = np.zeros((int(off[count]), 3), dtype=np.int32)
        capi.check(lib.cvx_job_nm_profile(self.al.h, self.j, first, count, off.ctypes.data, tri.ctypes.data, int(off[count]), C.byref(ms)))
        return off, tri, ms.value

    def text_all(self, ext_qstart=None, ext_qend=None):
        """cvx_job_text_all (ABI 9): text() and nm_profile_resident() of the whole job in one call.
        -> (list of dicts as text(), entry offsets uint64[n + 1], triples int32[entries, 3])"""
        n = self.n
        out = (capi.CvxAlignmentText * max(n, 1))()
        off = np.zeros(max(n, 1), dtype=np.uint64)
        nmoff = np.zeros(n + 1, dtype=np.uint64)
        nbytes = C.c_uint64()
        eq = np.ascontiguousarray(ext_qstart, dtype=np.int32) if ext_qstart is not None else None
        ee = np.ascontiguousarray(ext_qend, dtype=np.int32) if ext_qend is not None else None
        lib = self.al.lib
        lib.cvx_job_text_all.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.CvxAlignmentText),
                                         C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_void_p)]
        tp, np_ = C.c_void_p(), C.c_void_p()
        capi.check(lib.cvx_job_text_all(self.al.h, self.j, eq.ctypes.data if eq is not None else None,
                                        ee.ctypes.data if ee is not None else None, out, off.ctypes.data,
                                        C.byref(tp), C.byref(nbytes), nmoff.ctypes.data, C.byref(np_)))
        raw = (C.c_char * int(nbytes.value)).from_address(tp.value).raw if nbytes.value else b""
        res = []
        for i in range(n):
            t = out[i]
            d = {f: getattr(t, f) for f, _ in capi.CvxAlignmentText._fields_}
            d["score_bits"] = int(np.float32(t.score).view(np.uint32))
            o = int(off[i])
            d["cigar"] = raw[o:o + t.cigar_len].decode()
            d["md"] = raw[o + t.cigar_len + 1:o + t.cigar_len + 1 + t.md_len].decode()
            res.append(d)
        e = int(nmoff[n])
        tri = np.ctypeslib.as_array(C.cast(np_, C.POINTER(C.c_int32)), shape=(e * 3,)).reshape(e, 3).copy() if e else np.zeros((0, 3), dtype=np.int32)
        return res, nmoff, tri

    def nm_profile_resident(self, first: int = 0, count: Optional[int] = None):
        """cvx_job_nm_profile_resident (ABI 9): the same triples left in the job's page-locked memory (copied out here).
        -> (entry offsets uint64[count + 1], triples int32[entries, 3], kernel ms)"""
        count = self.n - first if count is None else count
        off = np.zeros(count + 1, dtype=np.uint64)
        ms = C.c_double()
        ptr = C.c_void_p()
        capi.check(self.al.lib.cvx_job_nm_profile_resident(self.al.h, self.j, first, count, off.ctypes.data, C.byref(ptr), C.byref(ms)))
        n = int(off[count])
        tri = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(n * 3,)).reshape(n, 3).copy() if n else np.zeros((0, 3), dtype=np.int32)
        return off, tri, ms.value

    def nm_regions(self, first: int = 0, count: Optional[int] = None):
        """cvx_job_nm_regions (after text()/text_raw()): the low-identity regions of the NM profile of the tiles
        [first, first + count) -- by default the whole job -- found on the device; no profile is written or copied.
        -> (offsets uint64[count + 1], regions int32[r, 4] = (ref_start, ref_stop, read_start, read_stop), open records
        NM_OPEN_DTYPE[count], kernel ms)"""
        count = self.n - first if count is None else count
        off = np.zeros(count + 1, dtype=np.uint64)
        opn = np.zeros(max(count, 0), dtype=NM_OPEN_DTYPE)
        ms = C.c_double()
        ptr = C.c_void_p()
        capi.check(self.al.lib.cvx_job_nm_regions(self.al.h, self.j, first, count, off.ctypes.data, C.byref(ptr), opn.ctypes.data, C.byref(ms)))
        n = int(off[count]) if count > 0 else 0
        reg = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(n * 4,)).reshape(n, 4).copy() if n else np.zeros((0, 4), dtype=np.int32)
        return off, reg, opn, ms.value

    def regions(self):
        """cvx_job_regions (a ConvexAlignHip(nm_regions=True) job, after wait()): the same regions of every tile as they came
        back with the job's results -- no text stage and no device call.
        -> (offsets uint64[n + 1], regions int32[r, 4], open records NM_OPEN_DTYPE[n]), copied out of the job's memory"""
        po, pr, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(self.al.lib.cvx_job_regions(self.al.h, self.j, C.byref(po), C.byref(pr), C.byref(pn)))
        n = self.n
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        r = int(off[n])
        reg = np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_int32)), shape=(r * 4,)).reshape(r, 4).copy() if r else np.zeros((0, 4), dtype=np.int32)
        opn = (np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint8)), shape=(n * NM_OPEN_DTYPE.itemsize,)).view(NM_OPEN_DTYPE).copy()
               if n else np.zeros(0, dtype=NM_OPEN_DTYPE))
        return off, reg, opn

    def checks(self):
        """cvx_job_checks (a ConvexAlignHip(nm_regions=True, inv_checks=True) job, after wait()): the inversion check of every
        region, parallel to regions()' regions, as it came back with them -- no device call.
        -> INV_CHECK_DTYPE[r], copied out of the job's memory; None for a job without a genome or without a region"""
        pc = C.c_void_p()
        capi.check(self.al.lib.cvx_job_checks(self.al.h, self.j, C.byref(pc)))
        if not pc.value:
            return None
        r = self.regions_info()["total"]
        return np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_uint8)), shape=(r * INV_CHECK_DTYPE.itemsize,)).view(INV_CHECK_DTYPE).copy()

    def regions_info(self) -> dict:
        """cvx_job_regions_info: regions of the job, regions the arena held when the device first wrote them, and how often
        the write ran again over a larger arena."""
        total, cap, again = C.c_uint64(), C.c_uint64(), C.c_int32()
        capi.check(self.al.lib.cvx_job_regions_info(self.al.h, self.j, C.byref(total), C.byref(cap), C.byref(again)))
        return {"total": int(total.value), "first_capacity": int(cap.value), "rewrites": int(again.value)}

    def texts_raw(self):
        """cvx_job_texts (a ConvexAlignHip(job_text=True) job, after wait()): records, offsets and strings as they came back with
        the job's results, external clips zero -- no text stream and no device call.
        -> (list of CvxAlignmentText copies, offsets uint64[n + 1], the text bytes), copied out of the job's memory"""
        pr, po, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        capi.check(self.al.lib.cvx_job_texts(self.al.h, self.j, C.byref(pr), C.byref(po), C.byref(pt)))
        n = self.n
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        recs = [capi.CvxAlignmentText.from_buffer_copy(C.string_at(pr.value + i * C.sizeof(capi.CvxAlignmentText), C.sizeof(capi.CvxAlignmentText)))
                for i in range(n)]
        raw = C.string_at(pt.value, int(off[n])) if int(off[n]) else b""
        return recs, off, raw

    def texts(self, ext_qstart=None, ext_qend=None) -> List[dict]:
        """-> the list of dicts Job.text() returns, from cvx_job_texts; with external clips (per tile, either may be None = zeros)
        every tile goes through cvx_text_reclip."""
        recs, off, raw = self.texts_raw()
        res = []
        for i in range(self.n):
            t = recs[i]
            o = int(off[i])
            cigar = raw[o:o + t.cigar_len]
            md = raw[o + t.cigar_len + 1:o + t.cigar_len + 1 + t.md_len]
            if ext_qstart is not None or ext_qend is not None:
                t, cigar = reclip(t, cigar, int(ext_qstart[i]) if ext_qstart is not None else 0,
                                  int(ext_qend[i]) if ext_qend is not None else 0, lib=self.al.lib)
            d = {f: getattr(t, f) for f, _ in capi.CvxAlignmentText._fields_}
            d["score_bits"] = int(np.float32(t.score).view(np.uint32))
            d["cigar"] = cigar.decode()
            d["md"] = md.decode()
            res.append(d)
        return res

    def texts_info(self) -> dict:
        """cvx_job_texts_info: bytes of the job's text, bytes the arena held when the device first wrote it, and how often the
        write ran again over a larger arena."""
        total, cap, again = C.c_uint64(), C.c_uint64(), C.c_int32()
        capi.check(self.al.lib.cvx_job_texts_info(self.al.h, self.j, C.byref(total), C.byref(cap), C.byref(again)))
        return {"total_bytes": int(total.value), "first_capacity": int(cap.value), "rewrites": int(again.value)}

    def release(self) -> None:
        if self.j:
            self.al.lib.cvx_job_release(self.al.h, self.j)
            self.j = None
            self.results = self.ops = None


def format_tileset(lib, tileset, idx, results, ops, n_threads: int = 0, scalar_twin: bool = False):
    """Host text stage (cvx_format_batch, all host threads) for tiles `idx` of a TileSet whose
    result records / ops arena are `results` / `ops` (numpy, RESULT_DTYPE).  Returns a list of
    dicts with the text-level Align fields (ret, score bits, CIGAR, MD, ...), no NM profile."""
    idx = np.asarray(idx, dtype=np.int64)
    n = len(idx)
    tab = np.ascontiguousarray(tileset.table()[idx])
    res = np.ascontiguousarray(results[idx])
    H = tileset.H[idx]
    caps = (4 * H + 64).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(caps)])
    cig = np.zeros(int(offs[-1]), dtype=np.uint8)
    md = np.zeros(int(offs[-1]), dtype=np.uint8)
    bufs = (capi.CvxTextBuffers * max(n, 1))()
    for k in range(n):
        bufs[k].cigar = cig.ctypes.data + int(offs[k])
        bufs[k].md = md.ctypes.data + int(offs[k])
        bufs[k].nm_triples = None
        bufs[k].cigar_cap = int(caps[k])
        bufs[k].md_cap = int(caps[k])
        bufs[k].nm_cap = 0
    out = (capi.CvxAlignmentText * max(n, 1))()
    capi.check(lib.cvx_format_batch_ex(n, res.ctypes.data_as(C.POINTER(capi.CvxResult)), ops.ctypes.data,
                                       tab.ctypes.data_as(C.POINTER(capi.CvxTile)), bufs, out, n_threads,
                                       capi.FORMAT_SCALAR_TWIN if scalar_twin else 0))
    texts = []
    for k in range(n):
        t = out[k]
        d = {f: getattr(t, f) for f, _ in capi.CvxAlignmentText._fields_}
        d["score_bits"] = int(np.float32(t.score).view(np.uint32))
        o = int(offs[k])
        d["cigar"] = cig[o:o + t.cigar_len].tobytes().decode() if t.cigar_len < caps[k] else None
        d["md"] = md[o:o + t.md_len].tobytes().decode() if t.md_len < caps[k] else None
        texts.append(d)
    return texts


def encode_genome(lib, seqs: Sequence[bytes]):
    """cvx_genome_encode: ngmlr's 4-bit reference encoding (host only).  -> (binref uint8[], nibbles, start table uint64[])"""
    n = len(seqs)
    lens = np.array([len(x) for x in seqs], dtype=np.uint64)
    arr = (C.c_char_p * max(n, 1))(*seqs)
    binref = np.zeros(int(lib.cvx_genome_encoded_bytes(n, lens.ctypes.data)), dtype=np.uint8)
    starts = np.zeros(n + 1, dtype=np.uint64)
    nib = C.c_uint64()
    ns = C.c_int32()
    capi.check(lib.cvx_genome_encode(n, arr, lens.ctypes.data, binref.ctypes.data, C.byref(nib), starts.ctypes.data, C.byref(ns)))
    return binref, int(nib.value), starts[:ns.value].copy()


class Genome:
    """An encoded reference genome resident in HBM (decode half): windows are decoded on the
    device -- the counterpart of SequenceProvider.DecodeRefSequenceExact (reference src/SequenceProvider.cpp:493-565)."""

    def __init__(self, aligner: ConvexAlignHip, binref: np.ndarray, nibbles: int, starts: np.ndarray):
        self.al = aligner
        self.g = C.c_void_p()
        b = np.ascontiguousarray(binref, dtype=np.uint8)
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        capi.check(aligner.lib.cvx_genome_upload(aligner.h, b.ctypes.data, int(nibbles), st.ctypes.data, len(st), C.byref(self.g)))

    def decode(self, positions, lengths) -> List[bytes]:
        """DecodeRefSequenceExact(position, length, corridor 0) for every window, `length` bytes each (the last a NUL)."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(ln.astype(np.int64))]).astype(np.uint64)
        out = np.zeros(int(off[-1]) + 8, dtype=np.uint8)
        capi.check(self.al.lib.cvx_genome_decode(self.al.h, self.g, len(pos), pos.ctypes.data, ln.ctypes.data, off.ctypes.data, out.ctypes.data))
        return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(pos))]

    def submit(self, tiles: Sequence, ref_positions) -> "Job":
        """cvx_submit_windows: the tiles' references are windows of this genome (tile.ref is not uploaded).
        `tiles`: as for ConvexAlignHip.submit, a synth.TileSet or a sequence of Tile objects."""
        if hasattr(tiles, "table"):
            tab = tiles.table()
            arr, keep = tab.ctypes.data_as(C.POINTER(capi.CvxTile)), (tiles, tab)
        else:
            arr, keep = self.al._pack(tiles)
        pos = np.ascontiguousarray(ref_positions, dtype=np.uint64)
        j = C.c_void_p()
        capi.check(self.al.lib.cvx_submit_windows(self.al.h, self.g, len(tiles), arr, pos.ctypes.data, C.byref(j)))
        return Job(self.al, j, len(tiles), (keep, pos))

    def free(self) -> None:
        if self.g:
            self.al.lib.cvx_genome_free(self.al.h, self.g)
            self.g = None


CANDIDATE_DTYPE = np.dtype([("location", np.uint64), ("score", np.float32), ("reverse", np.int32)])


class KmerIndex:
    """One unit of ngmlr's CompactPrefixTable resident in HBM, and CS::RunRead's candidate search over it for batches of
    (sub-)reads (search half; reference src/CS.cpp:57-149, 219-268, 324-398)."""

    def __init__(self, aligner: ConvexAlignHip, kmer_len: int, index_records: np.ndarray, locations: np.ndarray, unit_offset: int = 0):
        self.al = aligner
        self.ix = C.c_void_p()
        idx = np.ascontiguousarray(index_records)
        assert idx.dtype.itemsize == 5 and len(idx) == (1 << (2 * kmer_len)) + 2, "Index[4^k + 2], 5 packed bytes each"
        loc = np.ascontiguousarray(locations, dtype=np.uint32)
        capi.check(aligner.lib.cvx_index_upload(aligner.h, kmer_len, idx.ctypes.data, loc.ctypes.data, len(loc), unit_offset, C.byref(self.ix)))

    def search(self, reads: Sequence[bytes], sensitivity: float = 0.8, min_kmer_hits: float = 0.0, bin_shift: int = 4,
               first_bits: int = 0, extras: bool = False):
        """-> list (one per read) of CANDIDATE_DTYPE arrays in the reference's list order; None where the reference gives up.
        extras: also (max_hit float32[n], kmer_misses int32[n]) -- MappedRead::s and kCount of CS::RunRead."""
        n = len(reads)
        max_hit = np.zeros(max(n, 1), dtype=np.float32)
        misses = np.zeros(max(n, 1), dtype=np.int32)
        arr = (C.c_char_p * max(n, 1))(*reads)
        lens = np.array([len(r) for r in reads], dtype=np.int32)
        ncand = np.zeros(max(n, 1), dtype=np.int32)
        begin = np.zeros(max(n, 1), dtype=np.uint64)
        used = C.c_uint64()
        cap = 1 << 16
        while True:
            cands = np.zeros(cap, dtype=CANDIDATE_DTYPE)
            rc = self.al.lib.cvx_search_batch_ex(self.al.h, self.ix, n, arr, lens.ctypes.data, sensitivity, min_kmer_hits, bin_shift, first_bits,
                                                ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, cap, C.byref(used),
                                                max_hit.ctypes.data, misses.ctypes.data)
            if rc == -6 and used.value > cap:
                cap = int(used.value) + 64
                continue
            capi.check(rc)
            break
        lists = [None if ncand[i] < 0 else cands[int(begin[i]):int(begin[i]) + int(ncand[i])].copy() for i in range(n)]
        return (lists, max_hit[:n], misses[:n]) if extras else lists

    def last_attempts(self, n: int) -> np.ndarray:
        """cvx_search_last_attempts: table sizes tried by each of the first n reads of the handle's last search (int32[n]; more than
        one: the read's first attempt overflowed, CS::m_Overflows)."""
        attempts = np.zeros(max(n, 1), dtype=np.int32)
        capi.check(self.al.lib.cvx_search_last_attempts(self.al.h, n, attempts.ctypes.data))
        return attempts[:n]

    @staticmethod
    def make_arena(reads: Sequence[bytes], lib=None):
        """The reads back to back with a NUL behind each (cvx_search_batch_arena's input form) -> (arena uint8[], offsets uint64[n + 1],
        pinned handle or None).  lib: put the block into page-locked memory from cvx_host_alloc (the device then pulls it as it is)."""
        lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
        offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
        np.cumsum(lens + 1, out=offsets[1:])
        total = int(offsets[-1])
        blob = b"\0".join(reads) + b"\0" if len(reads) else b""
        pinned = None
        if lib is not None and total:
            p = C.c_void_p()
            if lib.cvx_host_alloc(total + 64, C.byref(p)) == 0:
                arena = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total + 64,))
                arena[:total] = np.frombuffer(blob, dtype=np.uint8)
                arena[total:] = 0
                pinned = (lib, p)
                return arena, offsets, pinned
        arena = np.frombuffer(blob + b"\0" * 64, dtype=np.uint8).copy()
        return arena, offsets, pinned

    def search_arena(self, arena: np.ndarray, offsets: np.ndarray, sensitivity: float = 0.8, min_kmer_hits: float = 0.0, bin_shift: int = 4,
                     first_bits: int = 0, cands: Optional[np.ndarray] = None):
        """cvx_search_batch_arena: reads that lie back to back -> flat outputs (n_cand int32[n], begin uint64[n], cands CANDIDATE_DTYPE[used],
        max_hit float32[n], kmer_misses int32[n]); read i's list = cands[begin[i] : begin[i] + n_cand[i]] (n_cand < 0: the reference gives up)."""
        n = len(offsets) - 1
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        max_hit = np.zeros(max(n, 1), dtype=np.float32)
        misses = np.zeros(max(n, 1), dtype=np.int32)
        ncand = np.zeros(max(n, 1), dtype=np.int32)
        begin = np.zeros(max(n, 1), dtype=np.uint64)
        used = C.c_uint64()
        if cands is None:
            cands = np.zeros(1 << 16, dtype=CANDIDATE_DTYPE)
        while True:
            rc = self.al.lib.cvx_search_batch_arena(self.al.h, self.ix, n, arena.ctypes.data, offsets.ctypes.data, sensitivity, min_kmer_hits, bin_shift, first_bits,
                                                   ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, len(cands), C.byref(used),
                                                   max_hit.ctypes.data, misses.ctypes.data)
            if rc == -6 and used.value > len(cands):
                cands = np.zeros(int(used.value) + int(used.value) // 8 + 64, dtype=CANDIDATE_DTYPE)
                continue
            capi.check(rc)
            break
        return ncand[:n], begin[:n], cands[:int(used.value)], max_hit[:n], misses[:n]

    def search_score_arena(self, genome: "Genome", arena: np.ndarray, offsets: np.ndarray, buffer_len: int, window_lead: int, max_cmrs: int,
                           sensitivity: float = 0.8, min_kmer_hits: float = 0.0, bin_shift: int = 4, first_bits: int = 0):
        """cvx_search_score_arena: search_arena and, in the same device call, every candidate scored against its window of the resident
        genome (position = location - window_lead, buffer_len characters of buffer) -> what search_arena returns plus
        (sw_scores float32[used], sw_status int32[used]), parallel to cands; status 1: no window at that position, 2: the read's list
        has max_cmrs entries or more (both score -1.0)."""
        n = len(offsets) - 1
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        max_hit = np.zeros(max(n, 1), dtype=np.float32)
        misses = np.zeros(max(n, 1), dtype=np.int32)
        ncand = np.zeros(max(n, 1), dtype=np.int32)
        begin = np.zeros(max(n, 1), dtype=np.uint64)
        used = C.c_uint64()
        cap = 1 << 16
        while True:
            cands = np.zeros(cap, dtype=CANDIDATE_DTYPE)
            sw_scores = np.zeros(cap, dtype=np.float32)
            sw_status = np.zeros(cap, dtype=np.int32)
            rc = self.al.lib.cvx_search_score_arena(self.al.h, self.ix, genome.g, n, arena.ctypes.data, offsets.ctypes.data, sensitivity, min_kmer_hits,
                                                   bin_shift, first_bits, buffer_len, window_lead, max_cmrs,
                                                   ncand.ctypes.data, begin.ctypes.data, cands.ctypes.data, cap, C.byref(used),
                                                   max_hit.ctypes.data, misses.ctypes.data, sw_scores.ctypes.data, sw_status.ctypes.data)
            if rc == -6 and used.value > cap:
                cap = int(used.value) + int(used.value) // 8 + 64
                continue
            capi.check(rc)
            break
        u = int(used.value)
        return ncand[:n], begin[:n], cands[:u], max_hit[:n], misses[:n], sw_scores[:u], sw_status[:u]

    def free(self) -> None:
        if self.ix:
            self.al.lib.cvx_index_free(self.al.h, self.ix)
            self.ix = None


class StrippedSWHip:
    """Mirror of the reference's StrippedSW for the scoring calls (src/StrippedSW.cpp:118-203):
    batch_score == BatchScore, single_score == SingleScore; alignment calls are not part of
    this backend.  GetScoreBatchSize() is 1024 in the reference (src/StrippedSW.h:53-55)."""

    def __init__(self, device: int = 0):
        self._al = ConvexAlignHip(device=device)
        self.lib = self._al.lib

    def get_score_batch_size(self) -> int:
        return 1024

    def batch_score(self, refs: Sequence[bytes], qrys: Sequence[bytes]) -> np.ndarray:
        n = len(refs)
        r = (C.c_char_p * max(n, 1))(*refs)
        q = (C.c_char_p * max(n, 1))(*qrys)
        out = np.zeros(max(n, 1), dtype=np.float32)
        capi.check(self.lib.cvx_score_batch(self._al.h, n, r, q, out.ctypes.data))
        return out[:n]

    def single_score(self, ref: bytes, qry: bytes) -> float:
        return float(self.batch_score([ref], [qry])[0])

    def submit_scores(self, refs: Sequence[bytes], qrys: Sequence[bytes]) -> "ScoreJob":
        """cvx_score_submit: the same scores as batch_score, split by shape into one launch per class; returns at once.
        The strings are copied before this returns."""
        n = len(refs)
        if len(qrys) != n:
            raise ValueError("submit_scores: %d refs, %d qrys" % (n, len(qrys)))
        r = (C.c_char_p * max(n, 1))(*refs)
        q = (C.c_char_p * max(n, 1))(*qrys)
        job = C.c_void_p()
        capi.check(self.lib.cvx_score_submit(self._al.h, n, r, q, C.byref(job)))
        return ScoreJob(self, job, n)

    def score_windows(self, genome: "Genome", reads, pairs):
        """cvx_score_windows: every pair scored against a window of the resident genome, both strings written on the device.
        reads: a sequence of bytes, or (arena, offsets) from KmerIndex.make_arena; pairs: (position, buffer_len, read, reverse)
        tuples or a WINDOW_DTYPE array.  -> (scores float32[n], status int32[n]); status 1 (score -1.0): the reference's
        DecodeRefSequence fails for that position."""
        arena, offsets, n_reads = _window_reads(reads)
        tab = _window_pairs(pairs)
        n = len(tab)
        scores = np.zeros(max(n, 1), dtype=np.float32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        capi.check(self.lib.cvx_score_windows(self._al.h, genome.g, n_reads, arena.ctypes.data, offsets.ctypes.data, n, tab.ctypes.data,
                                              scores.ctypes.data, status.ctypes.data))
        return scores[:n], status[:n]

    def submit_windows(self, genome: "Genome", reads, pairs) -> "ScoreJob":
        """cvx_score_windows_submit: the same, returning at once (the reads are copied before it returns); wait() gives the scores,
        -1.0 where the decode fails."""
        arena, offsets, n_reads = _window_reads(reads)
        tab = _window_pairs(pairs)
        job = C.c_void_p()
        capi.check(self.lib.cvx_score_windows_submit(self._al.h, genome.g, n_reads, arena.ctypes.data, offsets.ctypes.data, len(tab), tab.ctypes.data,
                                                     C.byref(job)))
        return ScoreJob(self, job, len(tab))

    def stage_windows(self, genome: "Genome", reads, pairs):
        """cvx_stage_windows: the strings the device would score -> (windows, queries, status), lists of bytes in pair order."""
        arena, offsets, n_reads = _window_reads(reads)
        tab = _window_pairs(pairs)
        return _stage_windows(lambda *out: self.lib.cvx_stage_windows(self._al.h, genome.g, n_reads, arena.ctypes.data, offsets.ctypes.data,
                                                                      len(tab), tab.ctypes.data, *out), tab, offsets)

    def stage_kernel_ms(self) -> float:
        """of that time, stage_score_windows_kernel alone (CVX_STAGE_SCORE_WINDOWS; 0 after a call on strings)"""
        ms = C.c_float()
        capi.check(self.lib.cvx_stage_kernel_ms(self._al.h, capi.STAGE_SCORE_WINDOWS, C.byref(ms)))
        return ms.value

    def kernel_ms(self) -> float:
        """device time of the kernels of the handle's last scoring call (cvx_stage_kernel_ms, CVX_STAGE_SCORE)"""
        ms = C.c_float()
        capi.check(self.lib.cvx_stage_kernel_ms(self._al.h, capi.STAGE_SCORE, C.byref(ms)))
        return ms.value

    def close(self) -> None:
        self._al.close()


WINDOW_DTYPE = np.dtype([("position", np.uint64), ("buffer_len", np.int32), ("read", np.int32), ("reverse", np.int32), ("pad", np.int32)])
assert WINDOW_DTYPE.itemsize == C.sizeof(capi.CvxScoreWindow)


def _window_reads(reads):
    if isinstance(reads, tuple) and len(reads) == 2 and isinstance(reads[0], np.ndarray):
        arena, offsets = reads
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        return np.ascontiguousarray(arena, dtype=np.uint8), offsets, len(offsets) - 1
    arena, offsets, _ = KmerIndex.make_arena(list(reads))
    return arena, offsets, len(offsets) - 1


def _window_pairs(pairs) -> np.ndarray:
    if isinstance(pairs, np.ndarray) and pairs.dtype == WINDOW_DTYPE:
        return np.ascontiguousarray(pairs)
    tab = np.zeros(len(pairs), dtype=WINDOW_DTYPE)
    for i, (position, buffer_len, read, reverse) in enumerate(pairs):
        tab[i] = (int(position) & 0xFFFFFFFFFFFFFFFF, buffer_len, read, 1 if reverse else 0, 0)
    return tab


def _stage_windows(call, tab, offsets):
    n = len(tab)
    ref_off = np.zeros(max(n, 1), dtype=np.uint64)
    qry_off = np.zeros(max(n, 1), dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    used = C.c_uint64()
    # every window is at most buffer_len characters, every query its read: an upper bound without asking first
    rl = (offsets[1:] - offsets[:-1]).astype(np.int64)
    cap = int(tab["buffer_len"].astype(np.int64).clip(0).sum() + rl[tab["read"].clip(0, max(len(rl) - 1, 0))].sum() + n + 64) if n and len(rl) else 64
    out = np.zeros(cap, dtype=np.uint8)
    capi.check(call(out.ctypes.data, cap, ref_off.ctypes.data, qry_off.ctypes.data, status.ctypes.data, C.byref(used)))
    blob = out[:int(used.value)].tobytes()

    def cstr(at):
        return blob[at:blob.index(b"\0", at)]
    return [cstr(int(ref_off[i])) for i in range(n)], [cstr(int(qry_off[i])) for i in range(n)], status[:n]


def stage_windows_host(lib, binref, nibbles, starts, reads, pairs):
    """cvx_stage_windows_host: the same strings built on the host from an encoded genome (no device)."""
    arena, offsets, n_reads = _window_reads(reads)
    tab = _window_pairs(pairs)
    b = np.ascontiguousarray(binref, dtype=np.uint8)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    return _stage_windows(lambda *out: lib.cvx_stage_windows_host(b.ctypes.data, int(nibbles), st.ctypes.data, len(st), n_reads, arena.ctypes.data,
                                                                  offsets.ctypes.data, len(tab), tab.ctypes.data, *out), tab, offsets)


SEGMENT_DTYPE = np.dtype([("read", np.int32), ("start", np.int32), ("flags", np.int32), ("reserved", np.int32)])
assert SEGMENT_DTYPE.itemsize == C.sizeof(capi.CvxReadSegment)


def _segments(segments) -> np.ndarray:
    if isinstance(segments, np.ndarray) and segments.dtype == SEGMENT_DTYPE:
        return np.ascontiguousarray(segments)
    tab = np.zeros(len(segments), dtype=SEGMENT_DTYPE)
    for i, (read, start, flags) in enumerate(segments):
        tab[i] = (read, start, flags, 0)
    return tab


def _stage_segments(call, lengths) -> List[bytes]:
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    n = len(ln)
    qry_off = np.zeros(max(n, 1), dtype=np.uint64)
    used = C.c_uint64()
    cap = int(ln.astype(np.int64).clip(0).sum())
    out = np.zeros(cap + 64, dtype=np.uint8)
    capi.check(call(ln.ctypes.data, out.ctypes.data, cap, qry_off.ctypes.data, C.byref(used)))
    assert int(used.value) == cap
    return [out[int(qry_off[i]):int(qry_off[i]) + int(ln[i])].tobytes() for i in range(n)]


def stage_segments_host(lib, reads, segments, lengths) -> List[bytes]:
    """cvx_stage_segments_host: the same strings built on the host the way extractReadSeq builds them (no device)."""
    arena, offsets, n_reads = _window_reads(reads)
    seg = _segments(segments)
    return _stage_segments(lambda *io: lib.cvx_stage_segments_host(n_reads, arena.ctypes.data, offsets.ctypes.data, len(seg), seg.ctypes.data, *io), lengths)


def genome_concat_len(lib, nibbles, starts) -> int:
    """cvx_genome_concat_len: GetConcatRefLen() of an encoded genome"""
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    out = C.c_uint64()
    capi.check(lib.cvx_genome_concat_len(int(nibbles), st.ctypes.data, len(st), C.byref(out)))
    return int(out.value)


class ScoreJob:
    """One cvx_score_submit in flight: poll() -> bool, wait() -> float32 scores in call order (releases the job)."""

    def __init__(self, owner: StrippedSWHip, job, n: int):
        self.owner, self.job, self.n = owner, job, n

    def poll(self) -> bool:
        rc = self.owner.lib.cvx_score_poll(self.job)
        if rc < 0:
            capi.check(rc)
        return rc == 1

    def wait(self) -> np.ndarray:
        if self.job is None:
            raise RuntimeError("ScoreJob.wait: already waited for")
        out = np.zeros(max(self.n, 1), dtype=np.float32)
        job, self.job = self.job, None
        capi.check(self.owner.lib.cvx_score_wait(job, out.ctypes.data))
        return out[:self.n]


class DeviceBatch:
    """Tiles resident in HBM; run() may be repeated (bench) before download."""

    def __init__(self, aligner: ConvexAlignHip, handle, tiles):
        self.al = aligner
        self.b = handle
        self.tiles = tiles
        self.results = None
        self.ops = None

    def run(self) -> capi.CvxTiming:
        capi.check(self.al.lib.cvx_batch_run(self.al.h, self.b))
        t = capi.CvxTiming()
        capi.check(self.al.lib.cvx_batch_timing(self.b, C.byref(t)))
        return t

    def launches(self) -> list:
        t = capi.CvxTiming()
        capi.check(self.al.lib.cvx_batch_timing(self.b, C.byref(t)))
        out = []
        for i in range(t.n_fill_launches):
            li = capi.CvxLaunchInfo()
            capi.check(self.al.lib.cvx_batch_launch_info(self.b, i, C.byref(li)))
            out.append({k: getattr(li, k) for k, _ in capi.CvxLaunchInfo._fields_})
        return out

    def download(self):
        n = len(self.tiles)
        total = C.c_uint64()
        capi.check(self.al.lib.cvx_batch_ops_total(self.b, C.byref(total)))
        res = (capi.CvxResult * max(n, 1))()
        ops = np.zeros(max(int(total.value), 1), dtype=np.uint32)
        used = C.c_uint64()
        capi.check(self.al.lib.cvx_batch_download(self.al.h, self.b, res, ops.ctypes.data,
                                                  len(ops), C.byref(used)))
        self.results = res
        self.ops = ops
        return res, ops

    def alignments(self, want_nm: bool = True) -> List[dict]:
        if self.results is None:
            self.download()
        return [format_alignment(self.al.lib, self.results[i], self.ops, t, want_nm, scalar_twin=self.al.scalar_twin)
                for i, t in enumerate(self.tiles)]

    def format_batch(self, n_threads: int = 0, want_nm: bool = True):
        """Host text stage for the whole batch in one threaded C call (cvx_format_batch).
        Returns (seconds, texts, cigar_buffers, md_buffers)."""
        import time
        if self.results is None:
            self.download()
        n = len(self.tiles)
        arr, keep = self.al._pack(self.tiles)
        bufs = (capi.CvxTextBuffers * max(n, 1))()
        store = []
        for i, t in enumerate(self.tiles):
            cap = 4 * t.H + 64
            cig = C.create_string_buffer(cap)
            md = C.create_string_buffer(cap)
            nm = np.zeros((2 * (t.H + 1) + 16, 3), dtype=np.int32) if want_nm else None
            store.append((cig, md, nm))
            bufs[i].cigar = C.addressof(cig)
            bufs[i].md = C.addressof(md)
            bufs[i].nm_triples = nm.ctypes.data if want_nm else None
            bufs[i].cigar_cap = cap
            bufs[i].md_cap = cap
            bufs[i].nm_cap = len(nm) if want_nm else 0
            bufs[i].ext_qstart = t.ext_qstart
            bufs[i].ext_qend = t.ext_qend
        out = (capi.CvxAlignmentText * max(n, 1))()
        t0 = time.perf_counter()
        capi.check(self.al.lib.cvx_format_batch_ex(n, self.results, self.ops.ctypes.data, arr, bufs, out, n_threads,
                                                   capi.FORMAT_SCALAR_TWIN if self.al.scalar_twin else 0))
        dt = time.perf_counter() - t0
        return dt, out, store

    def free(self) -> None:
        if self.b:
            self.al.lib.cvx_batch_free(self.al.h, self.b)
            self.b = None


def format_alignment(lib, res: capi.CvxResult, ops: np.ndarray, tile, want_nm: bool = True, scalar_twin: bool = False) -> dict:
    """Host text stage (cvx_format_alignment_ex) -> dict with the Align fields.  scalar_twin: the text stage of
    Convex::ConvexAlign (no N-clip block; cigar_op_count and sv_type come back as capi.NOT_WRITTEN)."""
    H, W = len(tile.qry), len(tile.ref)
    cap = 4 * H + 64
    txt = capi.CvxAlignmentText()
    for _ in range(3):
        cig = C.create_string_buffer(cap)
        md = C.create_string_buffer(cap)
        nm_cap = 2 * (H + 1) + W + 16
        nm = np.zeros((nm_cap, 3), dtype=np.int32)
        capi.check(lib.cvx_format_alignment_ex(C.byref(res), ops.ctypes.data, tile.ref, W, H,
                                               tile.ext_qstart, tile.ext_qend, cig, cap, md, cap,
                                               nm.ctypes.data if want_nm else None, nm_cap,
                                               capi.FORMAT_SCALAR_TWIN if scalar_twin else 0, C.byref(txt)))
        if txt.cigar_len < cap and txt.md_len < cap:
            break
        cap = max(txt.cigar_len, txt.md_len) + 64
    d = {k: getattr(txt, k) for k, _ in capi.CvxAlignmentText._fields_}
    d["score_bits"] = int(np.float32(txt.score).view(np.uint32))
    d["cigar"] = cig.value.decode()
    d["md"] = md.value.decode()
    # What the reference's consumer reads: detectMisalignment walks nmPerPosition[i] for
    # i < alignmentLength (src/AlignmentBuffer.cpp:1320-1321), although only txt.nm_count triples were
    # written (positions > 16, none for insertion columns); the rest of the caller's buffer is zero here.
    # The buffer it walks is the caller's: (read length + 1) * 2 entries (src/AlignmentBuffer.cpp:277), doubled by addPosition
    # while the written triples do not fit (src/ConvexAlignFast.cpp:79-92; ConvexAlignHip::Finish grows it the same way) -- an
    # alignment with more columns than that (long deletions under a scoring with cheap gaps) is read up to the buffer's end.
    align_cap = 2 * (H + 1)
    while align_cap < txt.nm_count:
        align_cap *= 2
    n = min(txt.alignment_length, align_cap, nm_cap) if (txt.ret >= 0 and want_nm) else 0
    d["nm_per_position"] = nm[:n].copy()
    d["nm_count"] = txt.nm_count      # triples actually written
    d["status"] = res.status
    d["fwd_score_bits"] = int(np.float32(res.score).view(np.uint32))
    d["best_x"] = res.best_ref_index
    d["best_y"] = res.best_read_index
    d["rc"] = 0
    return d
