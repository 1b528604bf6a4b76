"""Letter-code helpers.

The reference turns FASTA records into a float one-hot array with a per-base
Python loop (sequences.py:20-31, :101-117) and needs Biopython.  The HIP path
only needs the letters: these helpers go from plain strings to one byte per
base (0..3 = A,C,G,T, the map of sequences.py:9-17) and to the reference's
one-hot layout, in vectorised NumPy.  The FASTA reader below is a small
stand-alone parser (the reference delegates to Bio.SeqIO, sequences.py:33-52).
"""
import os

import numpy as np

_LUT = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _LUT[ord(_ch)] = _i
    _LUT[ord(_ch.lower())] = _i


PROTEIN = "ACDEFGHIKLMNPQRSTVWY"      # the 20 amino acids, alphabetical one-letter codes (an `input_dims=20` model)


def _lut(alphabet):
    if alphabet == "ACGT":
        return _LUT
    if len(set(alphabet.upper())) != len(alphabet) or not 1 <= len(alphabet) <= 64:
        raise Exception("alphabet: 1 to 64 distinct letters")
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(alphabet):
        lut[ord(ch.upper())] = i
        lut[ord(ch.lower())] = i
    return lut


def seqsToCodes(seqs, alphabet="ACGT"):
    """list of equal-length strings -> uint8 array (n, L) of codes 0..len(alphabet)-1 (DNA by default: 0..3 = A,C,G,T).
    Sequences containing other letters (e.g. N) raise, like the reference
    skips them at read time (sequences.py:47-51).  Another `alphabet` (e.g. sequences.PROTEIN) gives the codes of a
    model built with input_dims=len(alphabet)."""
    seqs = [s if isinstance(s, str) else str(s) for s in seqs]
    if len({len(s) for s in seqs}) > 1:
        raise Exception("all sequences must have the same length")
    raw = np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8).reshape(len(seqs), -1)
    codes = _lut(alphabet)[raw]
    if (codes >= len(alphabet)).any():
        raise Exception("sequences may only contain %s" % ", ".join(alphabet))
    return codes


def codesToOneHot(codes, input_dims=4):
    """(n, L) codes -> (n,1,input_dims,L) float32 one-hot, the layout of seqToOneHot (sequences.py:101-117)."""
    codes = np.asarray(codes)
    n, L = codes.shape
    out = np.zeros((n, 1, input_dims, L), dtype=np.float32)
    out[np.arange(n)[:, None], 0, codes, np.arange(L)[None, :]] = 1
    return out


def seqToOneHot(seqs):
    """Drop-in for secomo.seqToOneHot on plain strings (or objects whose str() is the sequence)."""
    return codesToOneHot(seqsToCodes([str(getattr(s, "seq", s)) for s in seqs]))


class FastaRecord(object):
    """Minimal stand-in for the Bio.SeqRecord objects the reference hands around
    (only .id, .description and .seq are used by secomo)."""

    __slots__ = ("id", "description", "seq")

    def __init__(self, id, description, seq):
        self.id = id
        self.description = description
        self.seq = seq

    def __len__(self):
        return len(self.seq)

    def __str__(self):
        return self.seq

    def __repr__(self):
        return "FastaRecord(id=%r, len=%d)" % (self.id, len(self.seq))


def _iterFasta(handle):
    header, chunks = None, []
    for line in handle:
        line = line.strip()
        if not line:
            continue
        if line.startswith(">"):
            if header is not None:
                yield header, "".join(chunks)
            header, chunks = line[1:], []
        elif header is not None:
            chunks.append(line)
    if header is not None:
        yield header, "".join(chunks)


def readSeqsFromFasta(filename):
    """Read a multi-FASTA file; records containing N/n are skipped with the
    reference's message (sequences.py:33-52).  Returns a list of FastaRecord."""
    seqs = []
    with open(filename) as f:
        for header, seq in _iterFasta(f):
            if "N" in seq or "n" in seq:
                print("skip sequence containing N")
                continue
            ident = header.split(None, 1)[0] if header.strip() else ""
            seqs.append(FastaRecord(ident, header, seq))
    return seqs


def writeFasta(records, filename, width=60):
    """Write records as multi-FASTA, 60 columns per line like Bio.SeqIO.write."""
    with open(filename, "w") as f:
        for r in records:
            f.write(">%s\n" % (r.description or r.id))
            s = str(r.seq)
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")
    return len(records)


def splitTrainingTest(filename, train_test_ratio, num_top_regions=None, randomize=True):
    """Split a FASTA file into <prefix>_train.fa / <prefix>_test.fa
    (sequences.py:54-98: the first int(n*ratio) indices of the permutation are the test set)."""
    seqs = readSeqsFromFasta(filename)
    if num_top_regions:
        seqs = seqs[:num_top_regions]
    if randomize:
        idx_permut = list(np.random.permutation(len(seqs)))
    else:
        idx_permut = list(range(len(seqs)))
    ntest = int(len(seqs) * train_test_ratio)
    itest, itrain = idx_permut[:ntest], idx_permut[ntest:]
    prefix = ".".join(filename.split(".")[:-1])
    writeFasta([seqs[i] for i in itrain], prefix + "_train.fa")
    writeFasta([seqs[i] for i in itest], prefix + "_test.fa")


def fastaToCodes(filename):
    """FASTA file -> uint8 codes (n, L) without building per-base Python objects:
    the packed-ingestion path of SURVEY 8(f)-2 (feed the result to CRBM.fit /
    freeEnergy / motifHitProbs, which upload 1 byte per base)."""
    return seqsToCodes([r.seq for r in readSeqsFromFasta(filename)])


# stream codes (CRBM.scanSites): the letters in either case, 4 = no letter for N and the IUPAC ambiguity codes
_STREAM_LUT = _LUT.copy()
for _ch in "NRYSWKMBDHVU":
    if _STREAM_LUT[ord(_ch)] == 255:
        _STREAM_LUT[ord(_ch)] = 4
        _STREAM_LUT[ord(_ch.lower())] = 4
STREAM_GAP = 4


def seqsToStream(seqs, names=None):
    """Strings of any length -> (stream, offsets, names) for CRBM.scanSites: `stream` is one uint8 array, the records'
    codes (0..3 = A,C,G,T in either case; 4 = no letter: N and the IUPAC ambiguity codes) with exactly one code 4
    between two records; `offsets` (int64, len(seqs) + 1) holds the stream positions of the record starts, the last
    entry closing the last record (record i is stream[offsets[i]:offsets[i+1] - 1]); `names` defaults to seq<i>.
    Any other character raises.  Records may be empty."""
    seqs = [s if isinstance(s, str) else str(getattr(s, "seq", s)) for s in seqs]
    if names is None:
        names = ["seq{:d}".format(i) for i in range(len(seqs))]
    names = list(names)
    if len(names) != len(seqs):
        raise ValueError("names: one per record")
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lengths + 1, out=offsets[1:])
    try:
        raw = np.frombuffer("\n".join(seqs).encode("ascii"), dtype=np.uint8)
    except UnicodeEncodeError:
        raise ValueError("sequences may only contain A, C, G, T, N and the IUPAC ambiguity codes")
    lut = _STREAM_LUT.copy()
    lut[ord("\n")] = 254                                     # the separators (a newline inside a record is refused below)
    stream = lut[raw]
    if stream.size:
        sep = np.zeros(stream.size, dtype=bool)
        sep[offsets[1:-1] - 1] = True
        if (stream[~sep] > 4).any() or (stream[sep] != 254).any():
            raise ValueError("sequences may only contain A, C, G, T, N and the IUPAC ambiguity codes")
        stream[sep] = STREAM_GAP
    return np.ascontiguousarray(stream), offsets, names


def fastaToStream(filename):
    """FASTA file -> (stream, offsets, names) of seqsToStream, names = the record ids.  Unlike readSeqsFromFasta the
    reader keeps records that contain N: scanning is what they are for."""
    ids, seqs = [], []
    with open(filename) as f:
        for header, seq in _iterFasta(f):
            ids.append(header.split(None, 1)[0] if header.strip() else "")
            seqs.append(seq)
    return seqsToStream(seqs, ids)


def readVcf(path, names):
    """The variants of a VCF file for CRBM.alleleEffects: dict of `seq` (int64, the index of CHROM in `names`, as
    fastaToStream returns them), `pos` (int64, 0-based), `ref` and `alt` (lists of strings), `line` (int64, the
    1-based line of the file a variant came from) and `skipped`, the counts of what was left out: 'symbolic' alleles
    (<...>, * and .), 'breakend' alleles ([ or ]) and records on 'unknown_contig's.  Plain text or .gz; # lines are
    skipped; a multi-allelic ALT gives one variant per allele.  INFO and FORMAT are not read."""
    import gzip
    index = {str(n): i for i, n in enumerate(names)}
    seq, pos, ref, alt, line = [], [], [], [], []
    skipped = {"symbolic": 0, "breakend": 0, "unknown_contig": 0}
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        for no, text in enumerate(f, 1):
            if text.startswith("#") or not text.strip():
                continue
            cols = text.rstrip("\r\n").split("\t")
            if len(cols) < 5:
                raise ValueError("%s line %d: a VCF record has at least five tab-separated columns" % (path, no))
            try:
                p = int(cols[1]) - 1
            except ValueError:
                raise ValueError("%s line %d: POS is not an integer" % (path, no))
            for a in cols[4].split(","):
                if "[" in a or "]" in a:
                    skipped["breakend"] += 1
                elif a.startswith("<") or a in ("*", ".", ""):
                    skipped["symbolic"] += 1
                elif cols[0] not in index:
                    skipped["unknown_contig"] += 1
                else:
                    seq.append(index[cols[0]]); pos.append(p); ref.append(cols[3]); alt.append(a); line.append(no)
    return {"seq": np.array(seq, np.int64), "pos": np.array(pos, np.int64), "ref": ref, "alt": alt,
            "line": np.array(line, np.int64), "skipped": skipped}


def shuffleStream(stream, seed):
    """The background of a stream for CRBM.scoreHistogram: the letters of every maximal run of letters (codes 0..3)
    permuted uniformly at random, every code 4 -- gaps and record separators -- where it was.  Each run, and with it
    each record, keeps its length and composition; dinucleotide frequencies are not preserved.  The same seed gives
    the same stream."""
    if not isinstance(stream, np.ndarray) or stream.dtype != np.uint8 or stream.ndim != 1:
        raise ValueError("stream must be a one-dimensional uint8 array of codes 0..4 (seqsToStream)")
    out = stream.copy()
    letter = stream < STREAM_GAP
    pos = np.flatnonzero(letter)
    if pos.size:
        run = np.cumsum(~letter)[pos]                        # the letters of a run have the same number of gaps before them
        order = np.lexsort((np.random.default_rng(seed).random(pos.size), run))
        out[pos] = stream[pos[order]]
    return out


def load_sample(filename=None):
    """One-hot sample data (sequences.py:120-134).  The reference ships an Oct4
    ChIP-seq FASTA inside its package; this package carries no data files, so
    the path must be given (or set CRBM_SAMPLE_FASTA)."""
    filename = filename or os.environ.get("CRBM_SAMPLE_FASTA")
    if not filename or not os.path.exists(filename):
        raise Exception("load_sample needs the path of a FASTA file (argument or CRBM_SAMPLE_FASTA)")
    return seqToOneHot(readSeqsFromFasta(filename))
