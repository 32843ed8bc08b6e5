"""Sequence assessment without a reference: sequences against the k-mers of the reads they came from, on the GPU.

A k-mer of a sequence that the reads do not support is an error (from these a consensus QV); a solid k-mer of the reads that the
sequences lack is lost sequence (from these completeness).  The reads are counted exactly (k <= 16), the k-mers counted at least
`min_count` times become a set on the device (default 0: the valley of the count histogram, because with reads at 10 % error the
k-mers their errors made would excuse the sequences' errors), every sequence is walked against it, and the set of the sequences' own
k-mers is compared with it.  The contract is in include/mhap_hip.h ("Sequence assessment without a reference").

    python -m mhap_amd.kmer_qv reads.fasta sequences.fasta [-k 16] [--no-rc] [--min-count N] [--table t.tsv] [--bed b.bed]

`mhap-hip-kmers --assess` does the same from the same entry points and prints the same line.
"""
import os
import sys

USAGE = ("Usage: python -m mhap_amd.kmer_qv <reads FASTA> <sequences FASTA> [-k 16] [--no-rc] [--min-count 0] [--table <file>] [--bed <file>] [--device 0]\n"
         "  -k           k-mer size, 1 to 16 (default 16)\n"
         "  --no-rc      k-mers as they are read instead of canonical\n"
         "  --min-count  a k-mer of the reads is solid when it is counted at least this often (default 0: the valley of the count histogram)\n"
         "  --table      write \"name\\tbases\\twindows\\tmissing\\truns\\tunsupported\\terror\\tqv\" per sequence and a total line\n"
         "  --bed        write \"name\\tbegin\\tend\" per stretch of bases that no supported k-mer covers\n"
         "  --device     HIP device ordinal (default 0)\n")


class Assessment:
    """What assess() returns.  rows, intervals, totals, error, qv: the KmerEval's; names: the sequences' names (None for a FastaData);
    solid, own, both: the members of the reads' solid set, of the sequences' own set and of both; completeness = both / solid;
    min_count: the threshold used; line: the summary line the tools print; write_table / write_bed: the two files."""

    def __init__(self, ev, reads_set, own_set, both):
        self._ev = ev
        self.k, self.names = ev.k, ev.names
        self.rows, self.intervals, self.totals = ev.rows, ev.intervals, ev.totals
        self.error, self.qv = ev.error, ev.qv
        self.solid, self.own, self.both = reads_set.members, own_set.members, both
        self.min_count = reads_set.min_count
        self.completeness = both / reads_set.members if reads_set.members else float("nan")
        self.line = ev.summary(reads_set, own_set, both)

    def write_table(self, path):
        self._ev.write_table(path)

    def write_bed(self, path):
        self._ev.write_bed(path)


def _count(ms, source, k, canonical):
    from .api import FastaData, FastaScan
    ms.kmer_count_begin(k, canonical)
    if isinstance(source, FastaData):
        ms.kmer_count_add(source)
        return None
    scan = FastaScan(os.fspath(source))
    ms.kmer_count_add_scan(scan)
    return scan


def assess(reads, sequences, k=16, canonical=True, min_count=0, device=0):
    """Assess `sequences` against the k-mers of `reads` (each a FastaData, or the path of a plain, gz or bz2 FASTA file, which goes
    through the streamed ingest): an Assessment."""
    from .api import FastaData, MhapParams, MinHashSearch
    with MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) as ms:
        scan = _count(ms, reads, k, canonical)
        reads_set = ms.kmer_count_finish_set(min_count)
        if scan is not None:
            scan.close()
        scan = _count(ms, sequences, k, canonical)
        own_set = ms.kmer_count_finish_set(1)
        try:
            ev = ms.kmer_set_eval(reads_set, sequences if isinstance(sequences, FastaData) else scan)
            both = ms.kmer_set_compare(reads_set, own_set)[2]
            return Assessment(ev, reads_set, own_set, both)
        finally:
            if scan is not None:
                scan.close()
            reads_set.close()
            own_set.close()


def _die(msg):
    sys.stderr.write(f"mhap_amd.kmer_qv: {msg}\n{USAGE}")
    return 1


def main(argv=None):
    args = sys.argv[1:] if argv is None else list(argv)
    k, canonical, min_count, device, table, bed, files = 16, True, 0, 0, None, None, []
    i = 0
    while i < len(args):
        a = args[i]
        if a in ("-h", "--help"):
            sys.stdout.write(USAGE)
            return 0
        if a in ("-k", "--min-count", "--table", "--bed", "--device"):
            if i + 1 >= len(args):
                return _die(f"option {a} requires a value")
            v = args[i + 1]
            i += 1
            if a in ("--table", "--bed"):
                table, bed = (v, bed) if a == "--table" else (table, v)
            else:
                try:
                    n = int(v, 10)
                except ValueError:
                    return _die(f"{a} takes an integer")
                if n < 0:
                    return _die(f"{a} takes an integer that is not negative")
                if a == "-k":
                    k = n
                elif a == "--min-count":
                    min_count = n
                else:
                    device = n
        elif a == "--no-rc":
            canonical = False
        elif a.startswith("-"):
            return _die(f"unknown option {a}")
        else:
            files.append(a)
        i += 1
    if len(files) != 2:
        return _die("two input files: the reads, then the sequences to assess")
    if k < 1 or k > 16:
        return _die(f"k-mer size must be from 1 to 16 (got {k})")
    from .api import MhapError
    try:
        res = assess(files[0], files[1], k=k, canonical=canonical, min_count=min_count, device=device)
        if table is not None:
            res.write_table(table)
        if bed is not None:
            res.write_bed(bed)
    except MhapError as e:
        sys.stderr.write(f"mhap_amd.kmer_qv: {e}\n")
        return 1
    sys.stderr.write(res.line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
