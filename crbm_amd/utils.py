"""Motif export, motif-site export and motif-match export.

secomo/utils.py:16-47 writes one file per motif through Bio.motifs.jaspar;
this writer produces the same text layouts without Biopython.  The plotting
helpers of the reference's utils.py (logos, scatter plots, violin plots) are
analysis code outside the hot path and are not rebuilt; the embedding behind its
t-SNE plots is (runTSNE, crbm_amd/tsne.py).
"""
import os

from .tsne import tsneEmbed

_ALPHABET = ("A", "C", "G", "T")


def formatMotif(pfm, name, fformat="jaspar"):
    """Text of one motif.  'jaspar': header line '>id name' and one bracketed row
    per letter; 'pfm': four bare rows; 'tab': letter<TAB>values rows."""
    rows = [["{0:6.2f}".format(float(v)) for v in pfm[a]] for a in range(4)]
    if fformat == "jaspar":
        lines = [">{0} {1}".format(name, name)]
        lines += ["{0} [{1}]".format(_ALPHABET[a], " ".join(rows[a])) for a in range(4)]
    elif fformat == "pfm":
        lines = [" ".join(rows[a]) for a in range(4)]
    elif fformat == "tab":
        lines = ["\t".join([_ALPHABET[a]] + [t.strip() for t in rows[a]]) for a in range(4)]
    else:
        raise ValueError("Unknown JASPAR format %s" % fformat)
    return "\n".join(lines) + "\n"


def saveMotifs(model, path, name="mot", fformat="jaspar"):
    """Save the model's PFMs, one file <name><i>.pfm per motif (utils.py:16-47;
    motif ids are 1-based in the header, 0-based in the file name, as there)."""
    pfms = model.getPFMs()
    if not os.path.exists(path):
        os.makedirs(path)
    for i, pfm in enumerate(pfms):
        with open(os.path.join(path, "{}{:d}.{}".format(name, i, "pfm")), "w") as f:
            f.write(formatMotif(pfm, name + str(i + 1), fformat))


_STRAND = {1: "+", -1: "-", 0: "."}


def saveSites(model, sites, filename, names=None, fformat="bed", name="mot"):
    """Write the records of CRBM.motifSites() to `filename`.  'bed': BED6 lines
    chrom, start, end = start + motif_length, name, score = prob, strand (+ - .),
    with chrom = names[seq] (e.g. the FASTA record ids) or 'seq<i>' and the motif
    named like saveMotifs' headers (<name><k+1>); 'tab': the same fields under a
    header line."""
    if fformat not in ("bed", "tab"):
        raise ValueError("Unknown site format %s" % fformat)
    M = model.motif_length
    lines = ["chrom\tstart\tend\tmotif\tprob\tstrand"] if fformat == "tab" else []
    for r in sites:
        seq, k, start = int(r["seq"]), int(r["motif"]), int(r["start"])
        chrom = names[seq] if names is not None else "seq{:d}".format(seq)
        lines.append("\t".join([chrom, str(start), str(start + M), "{}{:d}".format(name, k + 1),
                                "{:.6g}".format(float(r["prob"])), _STRAND[int(r["strand"])]]))
    with open(filename, "w") as f:
        f.write("".join(line + "\n" for line in lines))


def saveMatches(comparison, filename, evalue=10.0):
    """Write the matches of a MotifComparison (compareMotifs) with an E-value of at most `evalue` to a tab file under a
    header line: query, target, offset, strand (+ -), overlap, p-value, E-value, q-value; sorted by query, then p-value."""
    lines = ["query\ttarget\toffset\tstrand\toverlap\tpvalue\tevalue\tqvalue"]
    for r in comparison.matches(evalue=evalue):
        lines.append("\t".join([comparison.queries[int(r["query"])], comparison.targets[int(r["target"])], str(int(r["offset"])),
                                _STRAND[int(r["strand"])], str(int(r["overlap"]))] +
                               ["{:.6g}".format(float(r[f])) for f in ("pvalue", "evalue", "qvalue")]))
    with open(filename, "w") as f:
        f.write("".join(line + "\n" for line in lines))


def runTSNE(model, seqs, **kw):
    """t-SNE of the sequences by their motif abundances (utils.py:136-160): the
    largest hit probability per sequence and motif, motifHitProbs(seqs).max(axis=(2,3)),
    embedded in the plane by tsneEmbed (whose keyword arguments pass through).
    `seqs` is the one-hot array or (n, L) letter codes; returns (n, 2) float32."""
    return tsneEmbed(model, model.motifHitSummary(seqs, position_mean=False)["max"], **kw)
