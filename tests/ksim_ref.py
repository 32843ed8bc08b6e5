"""A literal transcription of J/main/KmerStatSimulator.java for the tests: java.util.Random through mhap_amd.roc.JavaRandom, the
LinkedList walk of getSequence as a list with a cursor, compareKmers with Python sets and BottomSketch through the oracle's
canonical murmur3_32 hashes, a stable signed sort and Java's merge loop.  Slow; for small runs only.  Line numbers in the comments.

Shared with the module under test, so the stdout comparisons cannot catch a bug in them: mhap_amd.kmer_sim's java_double
(Double.toString), jaccard_to_identity, _jdiv (IEEE division), _java_int ((int) of a double) and convert_to_fasta, and mhap_amd.roc's
JavaRandom and get_range_overlap.  tests/test_ksim_cpu.py checks those separately (the Double.toString table and random round trips,
the identity formula, the FASTA line breaks, nextDouble against Java's values)."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mhap_amd import kmer_sim, roc  # noqa: E402
import oracle_lib as O  # noqa: E402


class JavaException(Exception):
    pass


class KmerStatSimulator:
    def __init__(self, seed=0):
        self.kmer = -1
        self.overlap = 100
        self.reference = None          # a list of records (str), as `sequences` holds them
        self.requestedLength = 5000.0
        self.sharedCount = 0.0
        self.skipMers = {}
        self.totalTrials = 10000
        self.halfError = False
        self.generator = roc.JavaRandom(seed)
        self.out = []                  # stdout lines
        self.reads = []                # (role, read) in generation order, the test hook of this transcription
        self.randomJaccard, self.randomMinHash, self.randomMerCounts = [], [], []
        self.sharedJaccard, self.sharedMinHash, self.sharedMerCounts = [], [], []

    def buildRandomSequence(self, length):   # :154-161
        return "".join(self.getRandomBase(None) for _ in range(length))

    def compareKmers(self, first, second):   # :163-187
        firstSeqs, totalSeqs, shared = set(), set(), set()
        for i in range(0, len(first) - self.kmer + 1):
            fmer = first[i:i + self.kmer]
            if fmer not in self.skipMers:
                firstSeqs.add(fmer)
            totalSeqs.add(fmer)
        for i in range(0, len(second) - self.kmer + 1):
            smer = second[i:i + self.kmer]
            if smer in firstSeqs:
                shared.add(smer)
            else:
                totalSeqs.add(smer)
        self.sharedCount = float(len(shared))
        return kmer_sim._jdiv(len(shared), len(totalSeqs))

    def bottomSketch(self, s):   # BottomSketch(s, k, 1256, true)
        n = len(s) - self.kmer + 1
        if n < 0:
            raise JavaException(f"java.lang.NegativeArraySizeException: {n}")
        hashes = [int(x) for x in O.kmer_hashes32(s, self.kmer, do_rc=True)] if n > 0 else []
        k = min(1256, len(hashes))
        return sorted(hashes)[:k]

    def compareMinHash(self, first, second):   # :189-194, BottomSketch.jaccard
        a, b = self.bottomSketch(first), self.bottomSketch(second)
        k = min(len(a), len(b))
        i = j = inter = union = 0
        while union < k:
            if a[i] < b[j]:
                i += 1
            elif a[i] > b[j]:
                j += 1
            else:
                inter += 1
                i += 1
                j += 1
            union += 1
        return kmer_sim._jdiv(inter, k)

    def getRandomBase(self, toExclude):   # :204-225
        result = None
        while result is None:
            base = self.generator.next_double()
            if base < 0.25:
                result = "A"
            elif base < 0.5:
                result = "C"
            elif base < 0.75:
                result = "G"
            else:
                result = "T"
            if toExclude is not None and toExclude == result:
                result = None
        return result

    def getSequence(self, seqLength, firstPos, sequence, errorRate, insertionRate, deletionRate, substitutionRate, trimRight):   # :234-296
        firstSeq = sequence[firstPos:min(len(sequence), firstPos + 2 * seqLength)]
        if len(firstSeq) < 2 * seqLength:
            firstSeq += sequence[0:min(len(sequence), 2 * seqLength - len(firstSeq))]
        lst = list(firstSeq)     # the LinkedList; `cur` is the ListIterator's cursor (index of the element next() returns)
        cur = 0
        while cur < len(lst):
            i = lst[cur]
            cur += 1                                          # iter.next()
            if self.generator.next_double() < errorRate:
                errorType = self.generator.next_double()
                if errorType < substitutionRate:
                    lst[cur - 1] = self.getRandomBase(i)      # iter.set
                elif errorType < insertionRate + substitutionRate:
                    cur -= 1                                  # iter.previous()
                    lst.insert(cur, self.getRandomBase(None))  # iter.add: before the cursor, which moves past it
                    cur += 1
                else:
                    cur -= 1
                    del lst[cur]                              # iter.remove()
        firstSeq = "".join(lst)
        n = len(firstSeq)
        if trimRight:
            if n < seqLength:
                raise JavaException(f"java.lang.StringIndexOutOfBoundsException: begin 0, end {seqLength}, length {n}")
            return firstSeq[0:seqLength]
        if n < seqLength:
            raise JavaException(f"java.lang.StringIndexOutOfBoundsException: begin {n - seqLength}, end {n}, length {n}")
        return firstSeq[n - seqLength:n]

    def simulate(self, insertionRate, delRate, subRate):   # :317-461
        errorRate = insertionRate + delRate + subRate
        insertionPercentage = kmer_sim._jdiv(insertionRate, errorRate)
        deletionPercentage = kmer_sim._jdiv(delRate, errorRate)
        subPercentage = kmer_sim._jdiv(subRate, errorRate)
        if errorRate < 0 or errorRate > 1:
            raise JavaException("Error rate must be between 0 and 1")
        sequences = self.reference
        for i in range(self.totalTrials):
            sequenceLength = kmer_sim._java_int(self.requestedLength)
            firstPos = 0
            seqID = 0
            if self.reference is not None:
                sequence = None
                while sequence is None or len(sequence) < 4 * sequenceLength:
                    seqID = self.generator.next_int(len(sequences))
                    sequence = sequences[seqID]
                firstPos = self.generator.next_int(len(sequence))
            else:
                sequence = self.buildRandomSequence(sequenceLength * 4)
            firstSeq = self.getSequence(sequenceLength, firstPos, sequence, errorRate, insertionPercentage, deletionPercentage,
                                        subPercentage, False)
            self.reads.append((0, firstSeq))
            if self.kmer < 0:
                self.out.append(f">s{i} {seqID} {firstPos + sequenceLength}")
                self.out.append(kmer_sim.convert_to_fasta(firstSeq))
                continue
            offset = kmer_sim._java_int(self.requestedLength * 2 - self.overlap)
            secondPos = (firstPos + offset) % len(sequence)
            h = self.halfError
            secondSeq = self.getSequence(sequenceLength, secondPos, sequence, 0 if h else errorRate, 0 if h else insertionPercentage,
                                         0 if h else deletionPercentage, 0 if h else subPercentage, True)
            self.reads.append((1, secondSeq))
            if len(firstSeq) != len(secondSeq) or len(firstSeq) != self.requestedLength:
                raise JavaException(f"Error wrong length first: {len(firstSeq)} second: {len(secondSeq)} requested "
                                    f"{kmer_sim.java_double(self.requestedLength)}")
            self.sharedJaccard.append(self.compareKmers(firstSeq, secondSeq))
            self.sharedMinHash.append(self.compareMinHash(firstSeq, secondSeq))
            self.sharedMerCounts.append(self.sharedCount)
            if self.reference is not None:
                sequence = None
                secondSeqID = 0
                while sequence is None or len(sequence) < 2 * sequenceLength:
                    secondSeqID = self.generator.next_int(len(sequences))
                    sequence = sequences[secondSeqID]
                secondPos = self.generator.next_int(len(sequence))
                while seqID == secondSeqID and roc.get_range_overlap(firstPos, firstPos + sequenceLength, secondPos,
                                                                     secondPos + sequenceLength) > 0:
                    secondPos = self.generator.next_int(len(sequence))
                secondSeq = self.getSequence(sequenceLength, secondPos, sequence, 0 if h else errorRate, 0 if h else insertionPercentage,
                                             0 if h else deletionPercentage, 0 if h else subPercentage, True)
            else:
                secondSeq = self.buildRandomSequence(sequenceLength)
            self.reads.append((2, secondSeq))
            self.randomJaccard.append(self.compareKmers(firstSeq, secondSeq))
            self.randomMinHash.append(self.compareMinHash(firstSeq, secondSeq))
            self.randomMerCounts.append(self.sharedCount)
        if len(self.sharedMerCounts) == 0:
            return
        J = kmer_sim.java_double
        for i in range(self.totalTrials):
            self.out.append("\t".join(J(v) for v in (self.sharedMerCounts[i], self.sharedJaccard[i], self.sharedMinHash[i],
                                                      kmer_sim.jaccard_to_identity(self.sharedMinHash[i], self.kmer),
                                                      self.randomMerCounts[i], self.randomJaccard[i], self.randomMinHash[i])))
        for name, vals in (("Shared mer counts", self.sharedMerCounts), ("Shared jaccard", self.sharedJaccard),
                           ("Shared MinHash jaccard", self.sharedMinHash), ("Random mer counts", self.randomMerCounts),
                           ("Random jaccard", self.randomJaccard), ("Random MinHash jaccard", self.randomMinHash)):
            mean, sd = self.outputStats(vals)
            self.out.append(f"{name} stats: {J(mean)}\t{J(sd)}")

    @staticmethod
    def outputStats(values):   # :278-299
        mean = 0.0
        N = 0
        for d in values:
            N += 1
            mean += d
        mean = kmer_sim._jdiv(mean, N)
        variance = 0.0
        for d in values:
            variance += (d - mean) * (d - mean)
        variance = kmer_sim._jdiv(variance, N - 1)
        return mean, math.sqrt(variance) if variance >= 0 else math.nan


def run(trials, length, ins, dele, sub, k=-1, overlap=100, one_sided=False, reference=None, skip=None, seed=0):
    """The transcription's stdout for the given arguments (reference: records as str, already upper-cased with N removed)."""
    f = KmerStatSimulator(seed)
    f.totalTrials, f.requestedLength, f.kmer, f.overlap, f.halfError = trials, float(length), k, overlap, one_sided
    f.reference = reference
    f.skipMers = dict(skip or {})
    f.simulate(ins, dele, sub)
    return "".join(x + "\n" for x in f.out), f


def pair_stats(a, b, k, skip=()):
    """(shared, total, intersect) of one pair, as compareKmers / compareMinHash count them."""
    f = KmerStatSimulator()
    f.kmer = k
    f.skipMers = {s: 1 for s in skip}
    f.compareKmers(a, b)
    shared = int(f.sharedCount)
    total = len({a[i:i + k] for i in range(len(a) - k + 1)} | {b[i:i + k] for i in range(len(b) - k + 1)})
    # a segment shorter than k - 1 has no windows here (Java's BottomSketch would throw; the simulator never builds one)
    sa = f.bottomSketch(a) if len(a) >= k - 1 else []
    sb = f.bottomSketch(b) if len(b) >= k - 1 else []
    kk = min(len(sa), len(sb))
    i = j = inter = u = 0
    while u < kk:
        if sa[i] < sb[j]:
            i += 1
        elif sa[i] > sb[j]:
            j += 1
        else:
            inter += 1
            i += 1
            j += 1
        u += 1
    return shared, total, inter
