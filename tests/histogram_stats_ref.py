"""A line-for-line pure-Python restatement of GetHistogramStats.process() and toString() (J/main/GetHistogramStats.java:63-96), the
reference the C export mhap_histogram_stats is compared against bit for bit.  Python floats are IEEE doubles without contraction, as
Java's are; what Python does differently (an exception on division by zero, int arithmetic without overflow) is spelled out."""
import math

NUM_SD = 7


def _jdiv(a, b):
    """Java's double division: x / 0.0 is +-Infinity or NaN, not an exception."""
    a, b = float(a), float(b)
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def process(histogram, percent):
    """histogram: {int count: int number} (the TreeMap); returns (mean, stdev, cut)."""
    mean = 0.0
    variance = 0.0
    sum_ = 0.0
    total = 0
    for val in sorted(histogram):                   # for (int val : this.histogram.keySet())
        count = histogram[val]
        i = 0
        while i < count:                            # for (long i = 0; i < count; i++)
            total += 1
            delta = float(val) - mean
            mean += _jdiv(delta, total)
            variance += delta * (float(val) - mean)
            sum_ += float(val)
            i += 1
    variance = _jdiv(variance, total)
    stdev = math.sqrt(variance) if variance == variance else math.nan
    cut = 0
    running = 0.0
    for val in sorted(histogram):
        count = histogram[val]
        running += float(val) * float(count)        # (double) val * count
        if _jdiv(running, sum_) > percent:
            cut = val
            break
    return mean, stdev, cut


def to_string(mean, stdev, cut):
    from mhap_amd.roc import decimal_format
    return decimal_format(mean) + "\t" + decimal_format(stdev) + "\t" + "\t" + str(cut) + "\t" + decimal_format(mean + NUM_SD * stdev)
