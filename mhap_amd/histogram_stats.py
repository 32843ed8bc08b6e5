"""GetHistogramStats (J/main/GetHistogramStats.java): the mean and standard deviation of a k-mer count histogram, the count below which
`percent` of all k-mer occurrences fall, and mean + 7 sd — what to choose mhap-hip-kmers' --min-fraction (and mhap-hip's
--filter-threshold) with.

    python -m mhap_amd.histogram_stats <histogram file> <percent>

reads lines of "<count> <number of distinct k-mers with that count>" (the layout of `meryl -Dh`, and of `mhap-hip-kmers --histogram`
and KmerCounts.write_histogram) and prints GetHistogramStats' one stdout line, "mean \\t stdev \\t \\t cut \\t mean+7sd", through
Utils.DECIMAL_FORMAT.  Restated literally, line numbers in the comments: the file is read as Java reads it (a name ending in bz2 or gz
is decompressed; Integer.parseInt of column 0, Long.parseLong of column 1 into a TreeMap; any exception ends the reading with the rows
read so far, and percent keeps its default 0.99 then); process()'s Welford loop, one dependent step per k-mer, runs in C++
(mhap_histogram_stats) with Java's double rounding.  Deliberate deviations: where Java prints a stack trace this prints one line to
stderr; a percent that Double.parseDouble rejects, or a missing argument, ends the run with exit status 1 and a line on stderr (Java
dies with an uncaught exception, also status 1); of a concatenated gz or bz2 file only the first member is read, as Java's
commons-compress streams do.
"""
import bz2
import ctypes as C
import re
import sys
import zlib

import numpy as np

from .roc import decimal_format, java_split, parse_double, parse_int

NUM_SD = 7               # :38
DEFAULT_PERCENT = 0.99   # :40
_LONG = re.compile(r"[+-]?[0-9]+\Z")


def parse_long(s):
    """Long.parseLong: NumberFormatException -> ValueError."""
    if not _LONG.match(s) or not -(1 << 63) <= int(s) < (1 << 63):
        raise ValueError(f'For input string: "{s}"')
    return int(s)


def _java_lines(text):
    """BufferedReader.readLine over the whole text: lines end at \\n, \\r or \\r\\n; no empty line after the last terminator."""
    lines = re.split(r"\r\n|\r|\n", text)
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def _open_text(path):
    """Utils.getFile(fileName, null) (J/utils/Utils.java:228-262) read to the end: (text, error or None).  A decompression error keeps the
    text decompressed before it, so that the rows before it are read, as Java's stream would have delivered them."""
    with open(path, "rb") as fh:
        raw = fh.read()
    err = None
    if path.endswith("bz2"):
        d = bz2.BZ2Decompressor()
    elif path.endswith("gz"):
        d = zlib.decompressobj(16 + zlib.MAX_WBITS)
    else:
        d = None
    if d is None:
        data = raw
    else:
        try:
            data = d.decompress(raw)
            if not d.eof:
                err = f"{path}: unexpected end of the compressed stream"
        except (OSError, EOFError, zlib.error) as e:
            data, err = b"", f"{path}: {e}"
    return data.decode("utf-8", errors="replace"), err


def read_histogram(path):
    """The constructor's reading (:45-61): (TreeMap as a dict count -> number, percent taken, error message or None).  The rows read before
    an exception stay; after one, the percent argument is not taken (percent = p comes after the loop, inside the same try)."""
    histogram = {}
    try:
        text, err = _open_text(path)
    except OSError as e:
        return histogram, False, f"{path}: {e.strerror or e}"
    lines = _java_lines(text)
    if err is not None:   # (a stream that fails mid-way: the lines up to its last complete one)
        lines = lines[:-1] if text and text[-1] not in "\r\n" else lines
    for i, line in enumerate(lines):
        split = java_split(line)                        # :51
        try:
            val = parse_int(split[0])                   # :52
            if len(split) < 2:
                raise ValueError(f"Index 1 out of bounds for length {len(split)}")
            count = parse_long(split[1])                # :53
        except ValueError as e:
            return histogram, False, f"{path}: line {i + 1}: {e}"
        histogram[val] = count                          # :54 (a repeated count replaces the earlier one)
    if err is not None:
        return histogram, False, err
    return histogram, True, None


def histogram_stats(vals, numbers, percent):
    """process() (:63-90) on rows in TreeMap order (ascending, distinct counts): (mean, stdev, cut), by mhap_histogram_stats."""
    from .api import MhapError, load_library
    lib = load_library()
    v = np.ascontiguousarray(vals, dtype=np.int32)
    n = np.ascontiguousarray(numbers, dtype=np.int64)
    if v.shape != n.shape:
        raise ValueError("vals and numbers differ in length")
    mean, stdev, cut = C.c_double(), C.c_double(), C.c_int64()
    rc = lib.mhap_histogram_stats(v.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), C.c_int64(len(v)), C.c_double(percent),
                                  C.byref(mean), C.byref(stdev), C.byref(cut))
    if rc != 0:
        raise MhapError(f"mhap_histogram_stats failed ({rc})")
    return mean.value, stdev.value, cut.value


def format_line(mean, stdev, cut):
    """toString() (:92-96)."""
    return (decimal_format(mean) + "\t" + decimal_format(stdev) + "\t" + "\t" + str(cut) + "\t"
            + decimal_format(mean + NUM_SD * stdev))


def get_histogram_stats(path, percent):
    """The line main() prints for the file and percent, and the error message of the reading (None when it read to the end)."""
    histogram, ok, err = read_histogram(path)
    keys = sorted(histogram)                            # TreeMap<Integer, Long>: ascending signed int
    mean, stdev, cut = histogram_stats(keys, [histogram[k] for k in keys], percent if ok else DEFAULT_PERCENT)
    return format_line(mean, stdev, cut), err


def main(argv=None):
    args = sys.argv[1:] if argv is None else list(argv)
    if len(args) < 2:
        print("Usage: python -m mhap_amd.histogram_stats <histogram file> <percent>", file=sys.stderr)
        return 1
    try:
        percent = parse_double(args[1])                 # :99, before the file is opened
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    line, err = get_histogram_stats(args[0], percent)
    if err is not None:
        print(f"GetHistogramStats: {err}", file=sys.stderr)
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
