"""Homopolymer-compress reads on the GPU: `python -m mhap_amd.hpc reads.fasta -o compressed.fasta [--map map.tsv] [--device 0]` writes
every read with each run of equal bases collapsed to one, under its own name, one unwrapped line per read (an empty line for a read
that was empty), and with --map one line per read: `name raw_length compressed_length longest_run`, tab-separated.  One line on
stderr gives the counts.

Most long-read errors are runs of the wrong length, and reads with such errors still overlap once the runs are collapsed (minimap2
-H, Canu's HiFi mode, Flye and hifiasm search in that space).  `compress` is what `mhap-hip --hpc` does between reading the reads and
sketching them: the compressed reads go to the search under the same ids, and `HpcReads.expand` carries the records found there back to
raw coordinates through the map that the compression kept on the device.  The contract is the "homopolymer compression" section of
include/mhap_hip.h; tests/hpc_ref.py restates it.  A `-f` filter file for such a search is counted on the compressed reads too
(`mhap-hip-kmers --hpc`).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import api
from .api import _Session, _opt, _ptr


class HpcReads(_Session):
    """The compressed reads of a FastaData and their maps (mhap_hpc_compress / _info / _copy / _expand_records):

        with compress(fasta) as hp:
            records = search(hp.fasta)               # any search of the compressed reads, which keep their ids
            raw = hp.expand(records)                 # the same records on the raw reads

    .fasta: a FastaData of the compressed reads; .starts: every read's map back to back, read r's clen + 1 entries from
    .start_offsets[r] on (start_of(r) cuts them out); .raw_lengths; .counts: a dict of api.HPC_COUNTS.  handle: a MinHashSearch whose
    device and stream to use (else one is made and closed with the object)."""

    _prefix = "mhap_hpc"

    def __init__(self, fasta, handle=None, device=0, group_bases=0):
        self.raw_lengths = np.ascontiguousarray(fasta.lengths, np.int32)
        bases, ids = np.ascontiguousarray(fasta.bases, np.uint8), np.ascontiguousarray(fasta.ids, np.int64)
        offsets = np.ascontiguousarray(fasta.offsets, np.int64)
        n = len(ids)
        if len(offsets) != n or len(self.raw_lengths) != n:
            raise api.MhapError(f"HpcReads: {n} ids, {len(offsets)} offsets and {len(self.raw_lengths)} lengths")
        super().__init__(handle, device, lambda: self._ms._chk(self._lib.mhap_hpc_compress(
            self._ms._h, _opt(bases), len(bases), _opt(ids), _opt(offsets), _opt(self.raw_lengths), n, C.c_int64(group_bases), C.byref(self._s))))
        try:
            counts = np.zeros(len(api.HPC_COUNTS), np.int64)
            self._ms._chk(self._lib.mhap_hpc_info(self._s, _ptr(counts)))
            self.counts = dict(zip(api.HPC_COUNTS, counts.tolist()))
            total = self.counts["compressed_bases"]
            cbases, coff = np.zeros(total, np.uint8), np.zeros(n + 1, np.int64)
            clen, self.starts = np.zeros(n, np.int32), np.zeros(total + n, np.int32)
            self._ms._chk(self._lib.mhap_hpc_copy(self._s, _opt(cbases), _ptr(coff), _opt(clen), _opt(self.starts)))
        except Exception:
            self.close()
            raise
        self.fasta = api.FastaData(cbases, coff[:n], clen, ids)
        self.start_offsets = coff[:n] + np.arange(n, dtype=np.int64)

    def start_of(self, read_index):
        """The map of one read: clen + 1 raw positions, the last one the raw length."""
        if not 0 <= read_index < len(self.fasta):
            raise api.MhapError(f"HpcReads.start_of: read {read_index} is not among the {len(self.fasta)} reads")
        o = int(self.start_offsets[read_index])
        return self.starts[o:o + int(self.fasta.lengths[read_index]) + 1]

    def expand(self, records, to=None):
        """Records in compressed coordinates on the raw reads (mhap_hpc_expand_records): the `from` reads are this object's, the `to`
        reads those of `to` (another HpcReads on the same device; None: this one)."""
        records = np.ascontiguousarray(records, dtype=api.RECORD_DTYPE)
        out = np.zeros(len(records), api.RECORD_DTYPE)
        self._ms._chk(self._lib.mhap_hpc_expand_records(self._s, to._s if to is not None else None, _opt(records), len(records), _opt(out)))
        return out

    def times(self):
        """Milliseconds of the compression: upload, the two passes with the scan, the summing of the run counts, the whole call (mhap_hpc_times)."""
        ms = np.zeros(4, np.float64)
        self._ms._chk(self._lib.mhap_hpc_times(self._s, _ptr(ms)))
        return dict(zip(("upload", "passes", "counts", "call"), ms.tolist()))


def compress(fasta, handle=None, device=0, group_bases=0):
    """Homopolymer-compress the reads of a FastaData on the GPU: an HpcReads.  group_bases: the raw bases a group of reads may have
    (0: the library's default; tests make it small); the result does not depend on it."""
    return HpcReads(fasta, handle=handle, device=device, group_bases=group_bases)


def longest_runs(starts, start_offsets, clen):
    """The longest run of every read from the maps (0 for an empty read)."""
    out = np.zeros(len(clen), np.int64)
    for r, (o, c) in enumerate(zip(np.asarray(start_offsets).tolist(), np.asarray(clen).tolist())):
        if c:
            out[r] = int(np.diff(starts[o:o + c + 1]).max())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.hpc", description=__doc__.split("\n\n")[0])
    ap.add_argument("reads")
    ap.add_argument("-o", "--output", default=None, help="the FASTA file of the compressed reads (default: stdout)")
    ap.add_argument("--map", default=None, help="also write one line per read: name raw_length compressed_length longest_run")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    with api.FastaScan(a.reads) as scan:   # (the names; the bases come from FastaData, which keeps one byte per base)
        names = scan.info()[2]
    fasta = api.FastaData.from_file(a.reads)
    if len(names) != len(fasta):
        raise api.MhapError(f"{a.reads}: {len(names)} names for {len(fasta)} reads")
    with compress(fasta, device=a.device) as hp:
        c = hp.fasta
        raw = c.bases.tobytes()
        text = "".join(f">{name}\n{raw[o:o + n].decode('latin-1')}\n" for name, o, n in zip(names, c.offsets.tolist(), c.lengths.tolist()))
        if a.output:
            with open(a.output, "w") as fh:
                fh.write(text)
        else:
            sys.stdout.write(text)
        if a.map:
            runs = longest_runs(hp.starts, hp.start_offsets, c.lengths)
            with open(a.map, "w") as fh:
                fh.write("".join(f"{name}\t{L}\t{n}\t{m}\n" for name, L, n, m in zip(names, hp.raw_lengths.tolist(), c.lengths.tolist(), runs.tolist())))
        print(api.hpc_counts_line([hp.counts[k] for k in api.HPC_COUNTS]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
