"""
aln2counts stage on the MI355X: the drop-in for micall/core/aln2counts.py.

Input is aligned.csv (sam2aln's distinct merged reads with their counts).
Rows are taken in runs of equal (refname, qcut) -- the reference groups them
with itertools.groupby (aln2counts.py:884-887) -- and every run produces
amino-acid and nucleotide counts in coordinate-reference positions, the
mixture consensus at each cutoff, the insertions relative to the coordinate
reference and the consensus sequences that did not align.  Output files are
byte-identical to the reference's (tests/test_gpu_aln2counts.py).

Split of the work:
  device -- everything per read: 3-frame codon / base counting of a run,
            with the first row that touched each counter (k_a2c_count), and
            the grouping of inserted amino-acid strings (k_a2c_ins_hash /
            _verify / _gather around k_a2c_tab_count / _compact, the table the
            nucleotide variants share), csrc/mh_a2c.hip.  The first row
            replaces the reference's Counter insertion order, which decides
            most_common() ties.
  host   -- everything per run and O(reference length): consensus letters
            from the counters (numpy), the coordinate mapping with its local
            EmpHIV25 Gotoh alignments (run on the device by mh_gotoh_align)
            and the CSV text.

Public names (SequenceReport, InsertionWriter, SeedAmino, SeedNucleotide,
ReportAmino, format_cutoff, aln2counts) and their signatures are the
reference's, so callers and the reference's tests drive this module
unchanged.  Differences that never reach an output file:
  * the progress callback hears the start and the end of each run, not every
    1 % of the file (aln2counts.py:136-141);
  * the nucleotide variant counts that the reference computes and drops
    (aln2counts.py:346-375) are computed only when asked for
    (SequenceReport.count_variants / write_variants, aln2counts(variants_csv=),
    --variants_csv): the report write_nuc_variants was meant to write, counted
    on the device (mh_a2c_variants).  write_nuc_variants / nuc_variants_csv
    fail as the reference's do;
  * the codons count_aminos drops because they translate to no amino acid
    (aln2counts.py:595-603) are counted, as X, partial and del, only when
    asked for (SequenceReport.write_amino_detail, aln2counts(amino_detail_csv=),
    --amino_detail_csv): k_a2c_detail through mh_a2c_codon_detail;
  * the amino acids single reads link at chosen positions of a coordinate
    region, a report the reference does not have, are counted only when asked
    for (SequenceReport.count_linkage / write_linkage, aln2counts(linkage_csv=,
    linkage_positions=), --linkage_csv): k_a2c_link through mh_a2c_link;
  * which minority variants single reads carry together or keep apart, every
    pair of the variants a run's own counts select, another report the
    reference does not have, is counted only when asked for
    (SequenceReport.count_covariation / write_covariation,
    aln2counts(covariation_csv=), --covariation_csv): k_a2c_gram_bits and
    k_a2c_gram_pairs through mh_a2c_gram;
  * an InsertionWriter fed by a SequenceReport reads the run's rows from the
    device, so its nuc_seqs stays empty;
  * characters other than A C G T N - n, negative offsets and counts of 2**32
    or more raise NativeError.
When aligned_csv is the unchanged file this process's sam2aln() just wrote
from results that are still on the device (session.aligned_resident), the
file is not parsed: the rows, the codon extents and the bin lists are built
on the device from those results (mh_a2c_load_resident) and the reports are
the same bytes.  session.stats['aln2counts_source'] says which way a call
went ('device' or 'csv'); MICALL_ALN2COUNTS_RESIDENT=0 in the environment
forces the file path.
There is no CPU path: without libmicall_hip.so or a device the first call
raises NativeUnavailable.
"""
import argparse
import csv
import io
import json as jsonlib
import os
import re
from collections import Counter, namedtuple

import numpy as np

from . import _native
from . import projects as project_config
from . import session
from .translation import AMBIG, codon_chars, translate

AMINO_ALPHABET = 'ACDEFGHIKLMNPQRSTVWY*'
CONSEQ_MIXTURE_CUTOFFS = [0.01, 0.02, 0.05, 0.1, 0.2, 0.25]
GAP_OPEN_COORD, GAP_EXTEND_COORD = 40, 10
MAX_CUTOFF = 'MAX'

# Column order of every file the stage writes (the reference's output schema).
_SCHEMA = {
    'amino': ['seed', 'region', 'q-cutoff', 'query.aa.pos', 'refseq.aa.pos'] + list(AMINO_ALPHABET),
    'nuc': ['seed', 'region', 'q-cutoff', 'query.nuc.pos', 'refseq.nuc.pos'] + list('ACGT'),
    'nuc_detail': ['seed', 'region', 'q-cutoff', 'query.nuc.pos', 'refseq.nuc.pos'] + list('ACGT') +
                  ['N', 'del', 'clip', 'coverage'],
    'nuc_detail_ins': ['seed', 'region', 'q-cutoff', 'query.nuc.pos', 'refseq.nuc.pos'] + list('ACGT') +
                      ['N', 'del', 'clip', 'coverage', 'ins'],
    'nuc_detail_conc': ['overlap', 'mismatch', 'indel'],     # appended with concordance_csv
    'nuc_detail_strand': ['A_fwd', 'A_rev', 'C_fwd', 'C_rev', 'G_fwd', 'G_rev', 'T_fwd', 'T_rev',
                          'del_fwd', 'del_rev'],             # appended with strand_csv
    'amino_detail': ['seed', 'region', 'q-cutoff', 'query.aa.pos', 'refseq.aa.pos'] + list(AMINO_ALPHABET) +
                    ['X', 'partial', 'del', 'ins', 'clip', 'coverage'],
    'conseq': ['region', 'q-cutoff', 'consensus-percent-cutoff', 'offset', 'sequence'],
    'nuc_variants': ['seed', 'qcut', 'region', 'index', 'count', 'seq'],
    'failed': ['seed', 'region', 'qcut', 'queryseq', 'refseq'],
    'insert': ['seed', 'region', 'qcut', 'left', 'insert', 'count', 'before'],
    'coverage': ['avg_coverage', 'coverage_region', 'region_width'],
    'linkage': ['seed', 'region', 'q-cutoff', 'positions', 'haplotype', 'count', 'coverage'],
    'covariation': ['seed', 'q-cutoff', 'region.a', 'pos.a', 'aa.a', 'region.b', 'pos.b', 'aa.b', 'n', 'n.a',
                    'n.b', 'n.ab', 'direction', 'r2'],
}
LINKAGE_MAX_POSITIONS = 12            # positions of one linked set (mh_a2c_link: 5 key bits each)

# Covariation: the called characters of a codon in character order (the 21
# letters, then del), the bit of each in a column mask of mh_a2c_gram (codes
# 1..21 the letters, 24 del) and the mask of all of them.
COVARIATION_CALLED = AMINO_ALPHABET + '-'
COVARIATION_MAX_VARIANTS = 256        # two columns each at most: mh_a2c_gram takes 512
_COVAR_BIT = [1 << (k + 1) for k in range(len(AMINO_ALPHABET))] + [1 << 24]
_COVAR_CALLED = sum(_COVAR_BIT)

SLOT_REPORT, SLOT_INSERTS = 0, 1      # device row tables (mh_a2c slots) used here
_CODON_CHARS = codon_chars()
_NONE = np.uint32(0xffffffff)         # "no row touched this counter"
_AA = np.array(list(AMINO_ALPHABET))
# IUPAC letter of a set of bases, indexed by the mask A=1 C=2 G=4 T=8
_MIX = np.array(['', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'])
_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'gotoh_models.json')


def _csv_writer(handle, kind):
    return csv.DictWriter(handle, _SCHEMA[kind], lineterminator=os.linesep)


def _text(value):
    return value.decode('utf-8') if isinstance(value, bytes) else value


class _CoordinateAligner(object):
    """The module-level coordinate aligner of aln2counts.py:34-37 (local
    Gotoh, gap open 40 / extend 10, EmpHIV25 scores), evaluated on the device
    by mh_gotoh_align.  A seed's three translations meet the same coordinate
    references in every run, so results are kept (bounded) by input pair."""

    MEMO_LIMIT = 4096

    def __init__(self, gop, gep, is_global, model):
        with open(_MODELS) as f:
            spec = jsonlib.load(f)[model]
        self.gap_open_penalty, self.gap_extend_penalty = gop, gep
        self.is_global = is_global
        self.matrix, self.alphabet = spec['matrix'], spec['alphabet']
        self._outside = re.compile('[^%s]' % (self.alphabet,))
        self._memo = {}

    def forget(self):
        self._memo.clear()

    @staticmethod
    def _check(seq1, seq2):
        # gotoh2.py:74-96 asserts these (AssertionError as there)
        for name, seq in (('seq1', seq1), ('seq2', seq2)):
            if type(seq) is not str:
                raise AssertionError('%s must be a string' % name)
            if not seq:
                raise AssertionError('%s cannot be an empty string' % name)

    def align(self, seq1, seq2):
        """(aligned seq1, aligned seq2, score)."""
        return self.align_many([(seq1, seq2)])[0]

    def align_many(self, pairs):
        """align() of every pair; the pairs not seen before go to the device
        in one launch (mh_gotoh_align_batch).  A pair that fails raises, in
        pair order."""
        for seq1, seq2 in pairs:
            self._check(seq1, seq2)
        todo = list(dict.fromkeys(p for p in pairs if p not in self._memo))
        if todo:
            found = session.context().gotoh_align_many(
                [(self._outside.sub('?', a.upper()), self._outside.sub('?', b.upper()))
                 for a, b in todo],
                self.gap_open_penalty, self.gap_extend_penalty, self.is_global, self.alphabet,
                self.matrix)
            if len(self._memo) + len(todo) > self.MEMO_LIMIT:
                self._memo.clear()
            self._memo.update(zip(todo, found))
        out = [self._memo[p] for p in pairs]
        for result in out:
            if isinstance(result, Exception):
                raise result
        return out


aligner = _CoordinateAligner(GAP_OPEN_COORD, GAP_EXTEND_COORD, False, 'EmpHIV25')


# ---------------------------------------------------------------------------
# consensus letters and alignment walks
# ---------------------------------------------------------------------------
def _nuc_letters(cnt, first, cutoff):
    """The nucleotide consensus letter of every position at once
    (SeedNucleotide.get_consensus semantics, aln2counts.py:655-695).
    cnt / first: (positions, 6) over A C G T N -, `first` = first row that
    read the base (_NONE: never).  Returns (letters, coverage)."""
    present = first != _NONE
    total = cnt.sum(axis=1)
    acgt = present[:, :4]
    if cutoff == MAX_CUTOFF:
        score = np.where(acgt, cnt[:, :4], -1)
        mix = acgt & (score == score.max(axis=1, initial=-1)[:, None])
    else:
        mix = acgt & (cnt[:, :4] >= (total * cutoff)[:, None])
    letters = _MIX[mix.astype(np.int64) @ np.array([1, 2, 4, 8])]
    letters[letters == ''] = 'N'                  # every base below the cutoff
    # Only 'N' and / or '-' read: the first of them in most_common() order
    # is the one the removal of gaps and poor quality keeps.
    solo = present.any(axis=1) & ~acgt.any(axis=1)
    if solo.any():
        nc, dc = cnt[solo, 4], cnt[solo, 5]
        dash = present[solo, 5] & (~present[solo, 4] | (dc > nc) |
                                   ((dc == nc) & (first[solo, 5] < first[solo, 4])))
        kept = np.where(dash, dc, nc)
        ok = True if cutoff == MAX_CUTOFF else kept >= total[solo] * cutoff
        letters[solo] = np.where(ok, np.where(dash, '-', 'N'), 'N')
    letters[~present.any(axis=1)] = ''
    return letters, total


def _index_map(aligned_from, seq_from, aligned_to, seq_to):
    """{index in seq_to: index in seq_from} along an alignment: at every
    column where seq_from advances, the current seq_to index maps to it
    (the two walks of aln2counts.py:255-264 and :272-281)."""
    out = {}
    i = j = 0
    n_from, n_to = len(seq_from), len(seq_to)
    for a, b in zip(aligned_from, aligned_to):
        if i < n_from and a == seq_from[i]:
            out[j] = i
            i += 1
        if j < n_to and b == seq_to[j]:
            j += 1
    return out


def _fill(counter, letters, cnt, first):
    """Counter entries in first-row (insertion) order."""
    for k in np.argsort(first, kind='stable'):
        if first[k] == _NONE:
            break
        counter[letters[k]] = int(cnt[k])


# ---------------------------------------------------------------------------
# device counters of one run
# ---------------------------------------------------------------------------
_Run = namedtuple('_Run', 'ctx slot group ncod seed qcut')


class _Frame(object):
    """Device counters of one reading frame of one run."""

    def __init__(self, ctx, slot, g, frame, ncod):
        self.ncod = ncod
        if ncod:
            aa_cnt, aa_first, nt_cnt, nt_first = ctx.a2c_counts(slot, g, frame, ncod)
        else:
            aa_cnt = aa_first = np.zeros((0, 21), np.uint32)
            nt_cnt = nt_first = np.zeros((0, 18), np.uint32)
        self.aa_cnt = aa_cnt.astype(np.int64)
        self.aa_first = aa_first
        self.nt_cnt = nt_cnt.astype(np.int64).reshape(-1, 3, 6)
        self.nt_first = nt_first.reshape(-1, 3, 6)
        self.has = (aa_first != _NONE).any(axis=1)      # the codon's Counter is not empty
        self._consensus = None
        self.xpd = None       # X / partial / del per codon, once asked for (_codon_detail)

    def consensus(self):
        """Amino-acid consensus of the frame: the most counted amino acid of
        each codon, ties to the first one counted; '-' where none was."""
        if self._consensus is None:
            present = self.aa_first != _NONE
            score = np.where(present, self.aa_cnt, -1)
            tied = present & (score == score.max(axis=1, initial=-1)[:, None])
            pick = np.where(tied, self.aa_first, _NONE).argmin(axis=1)
            self._consensus = ''.join(np.where(self.has, _AA[pick], '-').tolist())
        return self._consensus

    def seed_amino(self, i):
        """A SeedAmino holding the device counts of codon i."""
        amino = SeedAmino(i)
        if i < self.ncod:
            _fill(amino.counts, AMINO_ALPHABET, self.aa_cnt[i], self.aa_first[i])
            for t, nuc in enumerate(amino.nucleotides):
                _fill(nuc.counts, 'ACGTN-', self.nt_cnt[i, t], self.nt_first[i, t])
        return amino


class _FrameAminos(object):
    """seed_aminos[frame] as a sequence of SeedAmino, materialised on access."""

    def __init__(self, frame, length):
        self._frame = frame
        self._len = length

    def __len__(self):
        return self._len

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._len))]
        if i < 0:
            i += self._len
        if not 0 <= i < self._len:
            raise IndexError('list index out of range')
        return self._frame.seed_amino(i)

    def __iter__(self):
        return (self[i] for i in range(self._len))


class _LazySeedAmino(object):
    """A report position's SeedAmino: its index now, its counts on access."""

    def __init__(self, frame, index):
        self.consensus_index = index
        self._frame = frame
        self._amino = None

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if self._amino is None:
            self._amino = self._frame.seed_amino(self.consensus_index)
        return getattr(self._amino, name)

    def __repr__(self):
        return repr(self._frame.seed_amino(self.consensus_index))


def _variant_window(conseq_index):
    """[start, end) in padded read positions of a coordinate region's
    variants, from the consensus codon of every coordinate position (-1:
    none): three times the first one to three times the last one plus one.
    A last codon of 0 counts as none (the reference's `or -1`,
    aln2counts.py:360), which empties the window."""
    placed = [int(k) for k in conseq_index if k >= 0]
    first = placed[0] if placed else 0
    last = (placed[-1] if placed else 0) or -1
    return 3 * first, 3 * (last + 1)


class _CoordinateMap(object):
    """Where one coordinate region sits in a run: the chosen reading frame,
    and per coordinate position the consensus codon index (-1: none)."""

    def __init__(self, frame=0, conseq_index=(), positions=()):
        self.frame = frame
        self.conseq_index = np.asarray(conseq_index, dtype=np.int64)
        self.positions = np.asarray(positions, dtype=np.int64)

    def __len__(self):
        return len(self.conseq_index)


def _check_linkage(positions, min_count=1):
    """The linked sets a caller gave, {region name: [set, ...]}, as lists of
    ints; ValueError naming the region and the set for one that is empty,
    longer than LINKAGE_MAX_POSITIONS, not strictly increasing or not made of
    integers >= 1, and for min_count < 1.  No device is touched."""
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
        raise ValueError('linkage: min_count must be an integer >= 1, not %r' % (min_count,))
    if not isinstance(positions, dict):
        raise ValueError('linkage: positions must map region names to lists of sets')
    checked = {}
    for region, sets in positions.items():
        if not isinstance(region, str) or not isinstance(sets, (list, tuple)):
            raise ValueError('linkage: region %r must be a name with a list of sets' % (region,))
        checked[region] = []
        for s, chosen in enumerate(sets):
            where = 'linkage: region %s, set %d %r' % (region, s, chosen)
            if not isinstance(chosen, (list, tuple)) or not chosen:
                raise ValueError(where + ' is empty or not a list')
            if len(chosen) > LINKAGE_MAX_POSITIONS:
                raise ValueError(where + ' holds more than %d positions' % LINKAGE_MAX_POSITIONS)
            if any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p < 1 for p in chosen):
                raise ValueError(where + ' must hold integers >= 1')
            if any(b <= a for a, b in zip(chosen, chosen[1:])):
                raise ValueError(where + ' is not strictly increasing')
            checked[region].append([int(p) for p in chosen])
    return checked


def _check_covariation(min_fraction=0.01, min_count=10, max_variants=COVARIATION_MAX_VARIANTS):
    """The thresholds of a covariation report as (min_fraction, min_count,
    max_variants); ValueError naming the one that is out of range:
    min_fraction outside (0, 1], min_count < 1, max_variants outside 1 ..
    256.  No device is touched."""
    if (isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating)) or
            not 0 < min_fraction <= 1):
        raise ValueError('covariation: min_fraction must be a number in (0, 1], not %r' % (min_fraction,))
    for name, value, top in (('min_count', min_count, None), ('max_variants', max_variants,
                                                              COVARIATION_MAX_VARIANTS)):
        if (isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1 or
                (top is not None and value > top)):
            raise ValueError('covariation: %s must be an integer %s, not %r' %
                             (name, '>= 1' if top is None else 'in 1 .. %d' % top, value))
    return float(min_fraction), int(min_count), int(max_variants)


def covariation_direction(n, na, nb, nab):
    """'+', '-' or '0': the two variants share rows more often, less often
    or exactly as often as independent ones would."""
    return '+' if n * nab > na * nb else '-' if n * nab < na * nb else '0'


def covariation_r2(n, na, nb, nab):
    """The squared correlation of the two indicators over the n rows called
    at both codons as '%.4f': integer numerator and denominator, one
    division; '' when a margin is empty or full."""
    bottom = na * (n - na) * nb * (n - nb)
    return '' if bottom == 0 else '%.4f' % ((n * nab - na * nb) ** 2 / bottom)


def _load_linkage(positions):
    """linkage_positions of aln2counts(): the mapping itself, or the path of
    a JSON file that holds only that mapping."""
    if isinstance(positions, (str, bytes, os.PathLike)):
        with open(positions) as f:
            positions = jsonlib.load(f)
    return positions


def _merge_linkage(parts):
    """Every rank's a2c_link results of one call, [(entries, coverage)], added
    up by (set, haplotype): the keys are exact, so equal haplotypes of a set
    are one entry whichever rank counted them.  Report order."""
    total, coverage = {}, None
    for found, cov in parts:
        coverage = list(cov) if coverage is None else [a + b for a, b in zip(coverage, cov)]
        for s, n, hap in found:
            total[s, hap] = total.get((s, hap), 0) + n
    return sorted(((s, n, hap) for (s, hap), n in total.items()), key=lambda e: (e[0], -e[1], e[2])), coverage


_LINK_RECORD = np.dtype([('set', '<i4'), ('count', '<i8'), ('hap', 'S%d' % LINKAGE_MAX_POSITIONS)])


def _pack_linkage(found, coverage):
    """A rank's a2c_link result on the wire: the per-set coverage, then
    fixed-size (set, count, haplotype) records."""
    rec = np.zeros(len(found), dtype=_LINK_RECORD)
    for k, (s, n, hap) in enumerate(found):
        rec[k] = (s, n, hap)
    return np.asarray(coverage, dtype='<i8').tobytes() + rec.tobytes()


def _unpack_linkage(blob, n_sets):
    coverage = np.frombuffer(blob[:8 * n_sets], dtype='<i8')
    rec = np.frombuffer(blob[8 * n_sets:], dtype=_LINK_RECORD)
    return [(int(r['set']), int(r['count']), bytes(r['hap'])) for r in rec], [int(c) for c in coverage]


# ---------------------------------------------------------------------------
# SequenceReport
# ---------------------------------------------------------------------------
class SequenceReport(object):
    """Counts and reports of one (refname, qcut) run of aligned reads
    (aln2counts.py:73-579).  read() a run, then call the write_* methods."""

    def __init__(self, insert_writer, projects, conseq_mixture_cutoffs):
        self.insert_writer = insert_writer
        self.projects = projects
        self.conseq_mixture_cutoffs = [MAX_CUTOFF] + list(conseq_mixture_cutoffs)
        self.callback = None

    def enable_callback(self, callback, file_size):
        """Report reading progress to callback(message, progress, max_progress)."""
        self.callback = callback
        self.callback_max = file_size
        callback(message='... extracting statistics from alignments', progress=0,
                 max_progress=file_size)

    def _pair_align(self, reference, query):
        """(aligned reference, aligned query, score) of the coordinate aligner;
        test doubles override this one method."""
        return aligner.align(_text(reference), _text(query))

    def _pair_align_many(self, pairs):
        """_pair_align of every (reference, query) pair: one device launch,
        unless a subclass (a test double) replaces _pair_align, which then
        answers each pair in turn."""
        if type(self)._pair_align is not SequenceReport._pair_align:
            return [self._pair_align(r, q) for r, q in pairs]
        return aligner.align_many([(_text(r), _text(q)) for r, q in pairs])

    # ---- reading a run ----
    def read(self, aligned_reads):
        """Start over with the rows given (dicts with refname, qcut, count,
        offset, seq); they go to the device as one run."""
        rows = list(aligned_reads)
        run = None
        if rows:
            ctx = session.context()
            ctx.a2c_load_rows(SLOT_REPORT, [r['seq'] for r in rows],
                              [int(r['offset']) for r in rows], [int(r['count']) for r in rows],
                              [0, len(rows)], _CODON_CHARS)
            run = _Run(ctx, SLOT_REPORT, 0, ctx.a2c_group(SLOT_REPORT, 0)['ncod'],
                       rows[0]['refname'], rows[0]['qcut'])
        self._start(run)

    def _read_group(self, ctx, slot, g):
        """read() of run g of a row table that is already on the device."""
        info = ctx.a2c_group(slot, g)
        self._start(_Run(ctx, slot, g, info['ncod'], info['refname'], info['qcut']))

    def _start(self, run):
        # state the write_* methods use; attribute names are the reference's
        for name in ('seed_aminos', 'reports', 'reading_frames', 'inserts', 'consensus',
                     'variants'):
            setattr(self, name, {})
        self._frames = None
        self._coord_maps = {}
        self._run = run
        self._variants_counted = False
        self.variant_stats = None
        self._job_detail = None
        self.linkage_unplaced = []
        self.linkage_stats = None
        self.covariation_stats = None
        if run is not None:
            self.seed, self.qcut = run.seed, run.qcut
            self.insert_writer.start_group(run.seed, run.qcut)
            self.insert_writer._attach(run.ctx, run.slot, run.group)
            self._frames = [_Frame(run.ctx, run.slot, run.group, f, run.ncod[f])
                            for f in range(3)]
            self.seed_aminos = {f: _FrameAminos(fr, fr.ncod) for f, fr in enumerate(self._frames)}
        if self.callback:
            self.callback(progress=self.callback_max)
        self.coordinate_refs = {}
        if self.seed_aminos:
            self.coordinate_refs = self.projects.getCoordinateReferences(self.seed)
            if not self.coordinate_refs:
                # no coordinate region: frame 0 covers the whole seed
                codons = -(-len(self.projects.getReference(self.seed)) // 3)
                frame0 = self._frames[0]
                self.seed_aminos[0] = _FrameAminos(frame0, max(frame0.ncod, codons))
        if self.coordinate_refs:
            self._locate_all({name: _text(ref) for name, ref in self.coordinate_refs.items()})

    def _locate_all(self, refs):
        """Coordinate position -> seed position -> consensus codon for every
        coordinate region of the seed (aln2counts.py:191-304), the regions'
        alignments batched in three launches:
          1. every frame's amino-acid consensus against every coordinate
             reference: a region's frame is the one scoring above
             min(covered codons, reference length), best first;
          2. the seed's three translations against each located region's
             reference: the best one maps coordinate -> seed positions;
          3. that translation against the chosen consensus: seed ->
             consensus positions."""
        frames = list(self.seed_aminos)
        conseqs = [self._frames[f].consensus() for f in frames]
        covered = int(self._frames[0].has.sum())
        for name in refs:
            self.consensus[name] = conseqs[0]           # kept if no frame aligns
        scores = iter(r[2] for r in self._pair_align_many(
            [(refs[name], c) for name in refs for c in conseqs]))
        chosen = {}
        for name, ref in refs.items():
            bar = min(covered, len(ref))
            for f, c in zip(frames, conseqs):
                score = next(scores)
                if score > bar:
                    bar, chosen[name] = score, (f, c)
        placed = {}
        if chosen:
            seed_nucs = self.projects.getReference(self.seed)
            translations = [translate(seed_nucs, offset=o, ambig_char='-') for o in range(3)]
            found = iter(self._pair_align_many(
                [(t, refs[name]) for name in chosen for t in translations]))
            for name in chosen:
                best_score, best = 0, None
                for t in translations:
                    aligned_seed, aligned_ref, score = next(found)
                    if score > best_score:
                        best_score, best = score, (t, aligned_seed, aligned_ref)
                t, aligned_seed, aligned_ref = best   # TypeError if none scored, as the reference
                placed[name] = (t, _index_map(aligned_seed, t, aligned_ref, refs[name]))
            final = self._pair_align_many([(placed[name][0], chosen[name][1]) for name in chosen])
        else:
            final = []
        blank = SeedAmino(None)
        finals = dict(zip(chosen, final))
        for name in refs:
            report, cmap = [], _CoordinateMap()
            if name in chosen:
                frame, consensus = chosen[name]
                self.reading_frames[name] = frame
                self.consensus[name] = consensus
                seed_aminos, ref_to_seed = placed[name]
                aligned_seed, aligned_conseq, _ = finals[name]
                # the aligner pads the left of a local alignment with '?'
                seed_to_conseq = _index_map(aligned_conseq.replace('?', '-'), consensus,
                                            aligned_seed, seed_aminos)
                unplaced = set(range(len(consensus)))
                self.inserts[name] = unplaced
                index, positions = [], []
                for ref_index in sorted(ref_to_seed):
                    k = seed_to_conseq.get(ref_to_seed[ref_index])
                    if k is None:
                        index.append(-1)
                        amino = blank
                    else:
                        index.append(k)
                        amino = _LazySeedAmino(self._frames[frame], k)
                        unplaced.remove(k)
                    positions.append(ref_index + 1)
                    report.append(ReportAmino(amino, ref_index + 1))
                cmap = _CoordinateMap(frame, index, positions)
            self.reports[name] = report
            self._coord_maps[name] = cmap

    def _gather(self, cmap, table, shape):
        """Rows of a per-codon counter table at the map's consensus codons
        (zeros where the coordinate position has none)."""
        out = np.zeros((len(cmap),) + shape, dtype=np.int64)
        hit = cmap.conseq_index >= 0
        if hit.any():
            out[hit] = table(self._frames[cmap.frame])[cmap.conseq_index[hit]]
        return out

    def _codon_detail(self, f):
        """(codons of frame f, 3) X, partial and del counts: the codons read
        there that translate to none of the 21 letters (mh_a2c_codon_detail;
        the first request after a load runs k_a2c_detail over every group of
        the slot, nothing is fetched before).  In a sharded job the tables
        are the job's, added up over the ranks (_job_detail)."""
        frame = self._frames[f]
        if frame.xpd is None:
            run = self._run
            if self._job_detail is not None:
                frame.xpd = self._job_detail[f]
            else:
                frame.xpd = run.ctx.a2c_codon_detail(run.slot, run.group, f, frame.ncod).astype(np.int64)
        return frame.xpd

    # ---- headers ----
    def write_amino_header(self, amino_file):
        _csv_writer(amino_file, 'amino').writeheader()

    def write_nuc_header(self, nuc_file):
        _csv_writer(nuc_file, 'nuc').writeheader()

    def write_consensus_header(self, conseq_file):
        _csv_writer(conseq_file, 'conseq').writeheader()

    def write_nuc_variants_header(self, nuc_variants_file):
        _csv_writer(nuc_variants_file, 'nuc_variants').writeheader()

    def write_failure_header(self, fail_file):
        _csv_writer(fail_file, 'failed').writeheader()

    def write_amino_detail_header(self, amino_detail_file):
        _csv_writer(amino_detail_file, 'amino_detail').writeheader()

    def write_nuc_detail_header(self, nuc_detail_file, insertions=False, concordance=False, strand=False):
        """insertions: the rows will end with the ins column; concordance:
        with overlap, mismatch, indel after it; strand: with the ten strand
        columns after those."""
        fields = _SCHEMA['nuc_detail_ins' if insertions else 'nuc_detail']
        if concordance:
            fields = fields + _SCHEMA['nuc_detail_conc']
        if strand:
            fields = fields + _SCHEMA['nuc_detail_strand']
        csv.DictWriter(nuc_detail_file, fields, lineterminator=os.linesep).writeheader()

    # ---- bodies ----
    def _amino_lines(self):
        """amino.csv's rows region by region, regions in name order: (name,
        the region's map, its (positions, 21) counts, its rows)."""
        for name in sorted(self.reports):
            cmap = self._coord_maps[name]
            if not len(cmap):
                continue
            counts = self._gather(cmap, lambda fr: fr.aa_cnt, (len(AMINO_ALPHABET),))
            query = ['' if k < 0 else str(k + 1) for k in cmap.conseq_index.tolist()]
            yield name, cmap, counts, [[self.seed, name, self.qcut, q, p] + c for q, p, c in
                                       zip(query, cmap.positions.tolist(), counts.tolist())]

    def write_amino_counts(self, amino_file, coverage_summary=None):
        """Amino-acid counts per coordinate position, regions in name order;
        the region with the highest mean count goes to coverage_summary."""
        out = csv.writer(amino_file, lineterminator=os.linesep)
        for name, cmap, counts, lines in self._amino_lines():
            out.writerows(lines)
            if coverage_summary is not None:
                mean = float(counts.sum()) / len(cmap)
                if mean > coverage_summary.get('avg_coverage', -1):
                    coverage_summary.update(avg_coverage=mean, coverage_region=name,
                                            region_width=len(cmap))

    def write_amino_detail(self, amino_detail_file, clipping=None, insertions=None):
        """amino.csv's rows (not in the reference) followed by what they leave
        out.  X, partial and del are the reads of the position's consensus
        codon, in the region's frame, that count_aminos drops because they
        translate to no amino acid: three of A C G T N with an ambiguous
        translation; a '-' or the gap between the mates beside a base (a
        deletion that is no multiple of three, a read end); all three bases
        deleted within the read.  coverage = the 21 letters + X + partial +
        del.  With k = query.aa.pos - 1 and f the region's frame the codon is
        consensus positions 3k - f + 1 .. 3k - f + 3 (write_nuc_detail's
        arithmetic): ins is the sum over them of the units that carry an
        insertion there at the row's cutoff, clip the largest of their
        soft-clip counts -- a lower bound of the units that clip any base of
        the codon, since a unit clipping two of them is one unit in each
        count.  clipping: {seed: {consensus position: count}} of sam2aln's
        clipping.csv; insertions: {seed: {(q-cutoff, pos): count}} of its
        conseq_ins.csv summed over the strings; None leaves the column
        empty.  Both are 0 without an entry or a query position."""
        clips = None if clipping is None else clipping.get(self.seed, {})
        inserts = None if insertions is None else insertions.get(self.seed, {})
        out = csv.writer(amino_detail_file, lineterminator=os.linesep)
        for name, cmap, counts, lines in self._amino_lines():
            f = cmap.frame
            xpd = self._gather(cmap, lambda fr: self._codon_detail(f), (3,))
            for line, k, three in zip(lines, cmap.conseq_index.tolist(), xpd.tolist()):
                codon = () if k < 0 else range(3 * k - f + 1, 3 * k - f + 4)
                ins = '' if inserts is None else sum(inserts.get((int(self.qcut), p), 0) for p in codon)
                clip = '' if clips is None else max([clips.get(p, 0) for p in codon], default=0)
                line += three + [ins, clip, sum(line[5:]) + sum(three)]
            out.writerows(lines)

    def _nuc_lines(self, classes):
        """nuc.csv's rows with the first `classes` of the A C G T N - counts
        of each nucleotide (in coordinate positions, or in seed positions when
        the seed has no coordinate region), and per row the reading frame of
        its region's map."""
        lines, frames = [], []
        if not self.coordinate_refs:
            n = len(self.seed_aminos[0])      # KeyError without reads, as the reference
            frame = self._frames[0]
            counts = np.zeros((n, 3, classes), dtype=np.int64)
            counts[:frame.ncod] = frame.nt_cnt[:, :, :classes]
            for codon, per_base in enumerate(counts.tolist()):
                lines.extend([self.seed, self.seed, self.qcut, 3 * codon + t + 1, ''] + acgt
                             for t, acgt in enumerate(per_base))
            frames = [0] * len(lines)
        else:
            for name, cmap in ((n, self._coord_maps[n]) for n in self.reports):
                counts = self._gather(cmap, lambda fr: fr.nt_cnt[:, :, :classes], (3, classes))
                for k, pos, per_base in zip(cmap.conseq_index.tolist(), cmap.positions.tolist(),
                                            counts.tolist()):
                    lines.extend([self.seed, name, self.qcut, '' if k < 0 else 3 * k + t + 1,
                                  3 * pos - 2 + t] + acgt for t, acgt in enumerate(per_base))
                frames += [cmap.frame] * (3 * len(cmap))
        return lines, frames

    def write_nuc_counts(self, nuc_file):
        """A/C/G/T counts per nucleotide: in coordinate positions, or in seed
        positions when the seed has no coordinate region."""
        csv.writer(nuc_file, lineterminator=os.linesep).writerows(self._nuc_lines(4)[0])

    def write_nuc_detail(self, nuc_detail_file, clipping=None, insertions=None, concordance=None,
                         strand=None):
        """nuc.csv's rows (not in the reference) followed by what they leave
        out: the N and deletion counts of the position, the units that
        soft-clip it, and coverage = A + C + G + T + N + del, the depth
        write_consensus tests against min_coverage.  clipping: {seed:
        {consensus position: count}} of sam2aln's clipping.csv, None to leave
        the clip column empty.  query.nuc.pos ignores the reading frame, so
        the consensus position of a row is query.nuc.pos - frame.
        insertions: {seed: {(q-cutoff, pos): count}} of sam2aln's
        conseq_ins.csv summed over the strings, None for no ins column; with
        it every row ends with ins, the units that carry an insertion after
        the row's consensus position at the row's cutoff.  concordance:
        {seed: {consensus position: (overlap, mismatch, indel)}} of sam2aln's
        concordance.csv, None for none; with it every row ends (after ins)
        with the pairs whose mates both align the row's consensus position and
        those that disagree there on a base or on an indel, 0 without an
        entry or a query position.  strand: {seed: {(q-cutoff, consensus
        position): the ten fwd and rev counts}} of sam2aln's strand.csv, None
        for none; with it every row ends (after those) with A_fwd, A_rev, ...
        del_fwd, del_rev of the row's consensus position at the row's cutoff,
        0 without an entry or a query position."""
        lines, frames = self._nuc_lines(6)
        strands = None if strand is None else strand.get(self.seed, {})
        concs = None if concordance is None else concordance.get(self.seed, {})
        clips = None if clipping is None else clipping.get(self.seed, {})
        inserts = None if insertions is None else insertions.get(self.seed, {})
        for line, f in zip(lines, frames):
            query = line[3]
            clip = '' if clips is None else 0 if query == '' else clips.get(query - f, 0)
            line[11:] = [clip, sum(line[5:11])]
            if inserts is not None:
                line.append(0 if query == '' else inserts.get((int(self.qcut), query - f), 0))
            if concs is not None:
                line.extend((0, 0, 0) if query == '' else concs.get(query - f, (0, 0, 0)))
            if strands is not None:
                line.extend(_NO_STRAND if query == '' else strands.get((int(self.qcut), query - f), _NO_STRAND))
        csv.writer(nuc_detail_file, lineterminator=os.linesep).writerows(lines)

    def write_consensus(self, conseq_file, min_coverage=100):
        """The nucleotide consensus of frame 0 from its first counted codon
        on, one row per mixture cutoff; bases read fewer than min_coverage
        times in lower case."""
        seed_aminos = self.seed_aminos[0]     # KeyError without reads, as the reference
        frame = self._frames[0]
        counted = np.flatnonzero(frame.has[:len(seed_aminos)])
        if not len(counted):
            return
        start = int(counted[0])
        cnt = frame.nt_cnt[start:].reshape(-1, 6)
        first = frame.nt_first[start:].reshape(-1, 6)
        out = _csv_writer(conseq_file, 'conseq')
        for cutoff in self.conseq_mixture_cutoffs:
            letters, depth = _nuc_letters(cnt, first, cutoff)
            letters = np.where(depth >= min_coverage, letters, np.char.lower(letters))
            out.writerow({'region': self.seed, 'q-cutoff': self.qcut,
                          'consensus-percent-cutoff': format_cutoff(cutoff),
                          'offset': start * 3, 'sequence': ''.join(letters.tolist())})

    def write_nuc_variants(self, nuc_variants_file):
        """The reference sorts dict.keys() in place here, which fails under
        Python 3 with AttributeError; so does this (no output either way)."""
        getattr(self.variants.keys(), 'sort')()

    def count_variants(self):
        """{coordinate region: [(count, clipped sequence), ...]} of the run
        just read: for every region a reading frame aligned to, the reads
        clipped to the region's consensus codons (aln2counts.py:346-375),
        equal ones added up, the projects' max_variants greatest by (count,
        sequence).  One device call for all regions, made once per read and
        only when asked (mh_a2c_variants; its figures in variant_stats)."""
        if self._variants_counted:
            return self.variants
        names = sorted(name for name, report in self.reports.items() if report)
        self.variants = {name: [] for name in names}
        if names and self._run is not None:
            windows = [_variant_window(self._coord_maps[name].conseq_index) for name in names]
            found, self.variant_stats = self._run.ctx.a2c_variants(
                self._run.slot, self._run.group, [w[0] for w in windows], [w[1] for w in windows],
                [len(self.coordinate_refs[name]) for name in names],
                [self.projects.getMaxVariants(name) for name in names])
            for k, count, seq in found:
                self.variants[names[k]].append((count, seq.decode('ascii')))
        self._variants_counted = True
        return self.variants

    def write_variants(self, variants_file):
        """The rows write_nuc_variants (aln2counts.py:537-549) was meant to
        write: regions in name order, each one's variants from index 0."""
        variants = self.count_variants()
        out = _csv_writer(variants_file, 'nuc_variants')
        out.writerows(dict(seed=self.seed, qcut=self.qcut, region=name, index=i, count=count, seq=seq)
                      for name in sorted(variants) for i, (count, seq) in enumerate(variants[name]))

    def write_linkage_header(self, linkage_file):
        _csv_writer(linkage_file, 'linkage').writeheader()

    def count_linkage(self, positions, min_count=1):
        """The amino acids the reads of the run just read link at chosen
        positions (not in the reference).  positions: {coordinate region:
        [set, ...]}, a set being 1 to 12 strictly increasing 1-based
        amino-acid positions of the region.  Returns [(region, set index,
        the set, [(haplotype, count), ...], coverage)] for every set placed in
        this run, regions in name order, sets as given.

        A set is placed when every position has a consensus codon in the
        region's map; the others are listed in linkage_unplaced as (region,
        set index).  A region that is not one of the seed's, or that no
        reading frame aligned to, is passed over.  A row's character at a
        position is the class amino_detail.csv counts its codon in -- the
        letter, X, '?' for partial, '-' for del -- and a row with a blank
        codon (padding only, or only the gap between the mates) at any
        position of a set does not count for the set.  Equal haplotypes add
        their counts up; the list holds those with count >= min_count, by
        count descending then haplotype ascending; coverage counts every row
        that counts, the dropped haplotypes' too.  One device call for all
        sets of the run (mh_a2c_link; its figures in linkage_stats), made
        only when asked.  In a sharded job every rank counts its own rows and
        the entries are added up by (set, haplotype)."""
        positions = _check_linkage(positions, min_count)
        self.linkage_unplaced = []
        self.linkage_stats = None
        refs = getattr(self, 'coordinate_refs', {})
        for name in sorted(positions):
            if name in refs:
                for s, chosen in enumerate(positions[name]):
                    if chosen[-1] > len(refs[name]):
                        raise ValueError('linkage: region %s, set %d %r reaches past the %d positions of '
                                         'the coordinate reference' % (name, s, chosen, len(refs[name])))
        asked, sets = [], []
        for name in sorted(positions):
            cmap = getattr(self, '_coord_maps', {}).get(name) if name in refs else None
            if cmap is None or not len(cmap):
                continue
            codon_of = dict(zip(cmap.positions.tolist(), cmap.conseq_index.tolist()))
            for s, chosen in enumerate(positions[name]):
                codons = [codon_of.get(p, -1) for p in chosen]
                if min(codons) < 0:
                    self.linkage_unplaced.append((name, s))
                else:
                    asked.append((name, s, chosen))
                    sets.append((cmap.frame, codons))
        run = getattr(self, '_run', None)
        if not sets or run is None:
            return []
        if _SHARD is not None and run.slot == SLOT_REPORT:
            from .sharded_io import _checked
            mine, self.linkage_stats = _checked(_SHARD, lambda: run.ctx.a2c_link(run.slot, run.group, sets, 1))
            found, coverage = _merge_linkage(
                _unpack_linkage(blob, len(sets))
                for blob in _SHARD.all_gather_bytes(_pack_linkage(mine, self.linkage_stats['coverage'])))
            found = [e for e in found if e[1] >= min_count]
        else:
            found, self.linkage_stats = run.ctx.a2c_link(run.slot, run.group, sets, min_count)
            coverage = self.linkage_stats['coverage']
        out = [(name, s, chosen, [], coverage[k]) for k, (name, s, chosen) in enumerate(asked)]
        for k, count, hap in found:
            out[k][3].append((hap.decode('ascii'), count))
        return out

    def write_linkage(self, linkage_file, positions, min_count=1):
        """linkage.csv's rows of this run: per placed set (count_linkage) one
        row per haplotype, with the set's positions joined by ';' and its
        coverage."""
        out = csv.writer(linkage_file, lineterminator=os.linesep)
        for name, _s, chosen, found, coverage in self.count_linkage(positions, min_count):
            where = ';'.join(str(p) for p in chosen)
            out.writerows([self.seed, name, self.qcut, where, hap, count, coverage] for hap, count in found)

    def write_covariation_header(self, covariation_file):
        _csv_writer(covariation_file, 'covariation').writeheader()

    def _covariation_candidates(self, min_fraction, min_count):
        """Every variant of the run as (-tally, region, position, character
        index, frame, consensus codon), from the tables the reports are made
        of: amino.csv's 21 counts and amino_detail.csv's del."""
        found = []
        for name in sorted(getattr(self, 'reports', {})):
            cmap = self._coord_maps.get(name)
            if cmap is None or not len(cmap):        # no reading frame aligned to it
                continue
            f = cmap.frame
            letters = self._gather(cmap, lambda fr: fr.aa_cnt, (len(AMINO_ALPHABET),))
            dels = self._gather(cmap, lambda fr: self._codon_detail(f), (3,))[:, 2]
            for tally, t_del, k, pos in zip(letters.tolist(), dels.tolist(), cmap.conseq_index.tolist(),
                                            cmap.positions.tolist()):
                tally.append(t_del)
                called = sum(tally)
                if k < 0 or not called:
                    continue
                major = tally.index(max(tally))      # ties: the earlier character
                found.extend((-t, name, pos, c, f, k) for c, t in enumerate(tally)
                             if c != major and t >= min_count and t >= min_fraction * called)
        return found

    def count_covariation(self, min_fraction=0.01, min_count=10, max_variants=COVARIATION_MAX_VARIANTS):
        """Which minority variants of the run just read travel together on
        single reads (not in the reference).  A row's character at a position
        is linkage's; the 21 letters and '-' (del) are *called*.  Per
        coordinate position with a consensus codon the major is the called
        character with the largest summed count (ties: the earlier of
        COVARIATION_CALLED); every other called character counted at least
        min_count times and at least min_fraction of the position's called
        rows is a variant.  More than max_variants (at most 256): the most
        counted stay, ties by (region name, position, character order), and
        covariation_stats['dropped'] says how many went.

        Returns one record per pair a < b of the kept variants, ordered by
        (region name, position, character order), that sit on different
        (frame, consensus codon) -- two regions of one seed pair up too --
        and have n >= min_count: (region.a, pos.a, aa.a, region.b, pos.b,
        aa.b, n, n.a, n.b, n.ab), over the rows called at both codons their
        summed count and those carrying a's character, b's, and both.

        The variants come from the tables amino.csv and amino_detail.csv are
        made of (in a sharded job the job's); the pairs from one device call
        (mh_a2c_gram; its figures in covariation_stats['native']) with one
        "called" column per distinct codon and one column per variant, made
        only when asked and only when two variants are kept.  In a sharded job
        every rank computes the matrix of its own rows and the matrices are
        added."""
        min_fraction, min_count, max_variants = _check_covariation(min_fraction, min_count, max_variants)
        self.covariation_stats = dict(variants=0, dropped=0, columns=0, pairs=0, native=None)
        run = getattr(self, '_run', None)
        if run is None:
            return []
        found = sorted(self._covariation_candidates(min_fraction, min_count))
        kept = sorted(v[1:] for v in found[:max_variants])
        self.covariation_stats.update(variants=len(kept), dropped=len(found) - len(kept))
        if len(kept) < 2:
            return []
        site = {}
        for _name, _pos, _c, f, k in kept:
            site.setdefault((f, k), len(site))
        cols = [(f, k, _COVAR_CALLED) for f, k in site] + [(f, k, _COVAR_BIT[c]) for _n, _p, c, f, k in kept]
        if _SHARD is not None and run.slot == SLOT_REPORT:
            from .sharded_io import _checked
            mine, native = _checked(_SHARD, lambda: run.ctx.a2c_gram(run.slot, run.group, cols))
            gram = sum(np.frombuffer(blob, dtype='<i8').reshape(len(cols), len(cols))
                       for blob in _SHARD.all_gather_bytes(mine.astype('<i8').tobytes()))
        else:
            gram, native = run.ctx.a2c_gram(run.slot, run.group, cols)
        gram = gram.tolist()
        out = []
        for i, a in enumerate(kept):
            sa, va = site[a[3:]], len(site) + i
            for j in range(i + 1, len(kept)):
                b = kept[j]
                sb, vb = site[b[3:]], len(site) + j
                n = gram[sa][sb]
                if sa != sb and n >= min_count:
                    out.append((a[0], a[1], COVARIATION_CALLED[a[2]], b[0], b[1], COVARIATION_CALLED[b[2]],
                                n, gram[va][sb], gram[sa][vb], gram[va][vb]))
        self.covariation_stats.update(columns=len(cols), pairs=len(out), native=native)
        return out

    def write_covariation(self, covariation_file, min_fraction=0.01, min_count=10,
                          max_variants=COVARIATION_MAX_VARIANTS):
        """covariation.csv's rows of this run: per pair (count_covariation)
        the four counts, direction ('+', '-' or '0' as n * n.ab is above,
        below or equal to n.a * n.b) and r2."""
        out = csv.writer(covariation_file, lineterminator=os.linesep)
        out.writerows([self.seed, self.qcut] + list(r) + [covariation_direction(*r[6:]), covariation_r2(*r[6:])]
                      for r in self.count_covariation(min_fraction, min_count, max_variants))

    def write_failure(self, fail_file):
        """One row per coordinate region that no reading frame aligned to."""
        out = _csv_writer(fail_file, 'failed')
        out.writerows(dict(seed=self.seed, region=name, qcut=self.qcut,
                           queryseq=self.consensus[name],
                           refseq=self.projects.getReference(name))
                      for name, report in self.reports.items() if not report)

    def write_insertions(self):
        for name in self.inserts:
            self.insert_writer.write(self.inserts[name], name, self.reading_frames[name],
                                     self.reports[name])


# ---------------------------------------------------------------------------
# per-codon / per-base counters (the reference's object API)
# ---------------------------------------------------------------------------
class SeedNucleotide(object):
    """Counts of the letters read at one nucleotide position."""

    def __init__(self):
        self.counts = Counter()

    def count_nucleotides(self, nuc_seq, count):
        # 'n' marks the unread gap between the forward and the reverse read
        if nuc_seq == 'n':
            return
        self.counts[nuc_seq] += count

    def get_report(self):
        return ','.join(str(self.counts[base]) for base in 'ACGT')

    def get_consensus(self, mixture_cutoff):
        """Consensus letter at a mixture cutoff (a fraction, or MAX_CUTOFF for
        the most counted bases only); a tie or a mixture is an IUPAC code.
        'N' and '-' count only when nothing else was read."""
        if not self.counts:
            return ''
        ranked = self.counts.most_common()
        informative = [pair for pair in ranked if pair[0] not in 'N-']
        candidates = informative or ranked[:1]
        if mixture_cutoff == MAX_CUTOFF:
            floor = candidates[0][1]
        else:
            floor = sum(self.counts.values()) * mixture_cutoff
        chosen = sorted(base for base, n in candidates if n >= floor)
        if not chosen:
            return 'N'
        return chosen[0] if len(chosen) == 1 else AMBIG[''.join(chosen)]


class SeedAmino(object):
    """Counts of the amino acids read at one codon, plus its three bases."""

    def __init__(self, consensus_index):
        self.consensus_index = consensus_index
        self.counts = Counter()
        self.nucleotides = [SeedNucleotide(), SeedNucleotide(), SeedNucleotide()]

    def __repr__(self):
        return '%s(%s): %s' % (type(self).__name__, self.consensus_index, self.counts)

    def count_aminos(self, codon_seq, count):
        amino = translate(codon_seq.upper())
        if amino in AMINO_ALPHABET:
            self.counts[amino] += count
        for k, nuc in enumerate(self.nucleotides):
            nuc.count_nucleotides(codon_seq[k], count)

    def get_report(self):
        return ','.join(str(self.counts[a]) for a in AMINO_ALPHABET)

    def get_consensus(self):
        top = self.counts.most_common(1)
        return top[0][0] if top else '-'


class ReportAmino(object):
    """A coordinate position (1-based) and the SeedAmino reported there."""

    __slots__ = ('seed_amino', 'position')

    def __init__(self, seed_amino, position):
        self.seed_amino, self.position = seed_amino, position

    def __repr__(self):
        return '%s(%r, %s)' % (type(self).__name__, self.seed_amino, self.position)


# ---------------------------------------------------------------------------
# insertions
# ---------------------------------------------------------------------------
def _ranges(indices):
    """Sorted indices -> [left, right) runs of consecutive values."""
    runs = []
    for k in sorted(indices):
        if runs and runs[-1][1] == k:
            runs[-1][1] = k + 1
        else:
            runs.append([k, k + 1])
    return runs


class InsertionWriter(object):
    """Writes the amino-acid strings read at consensus codons that have no
    coordinate position (insert.csv).  The counting over the reads runs on
    the device: over the run a SequenceReport attached, or over the reads
    given to add_nuc_read."""

    def __init__(self, insert_file):
        self._file = insert_file
        self.insert_writer = _csv_writer(insert_file, 'insert')
        self.insert_writer.writeheader()
        self.nuc_seqs = Counter()
        self._source = None

    def start_group(self, seed, qcut):
        self.seed, self.qcut = seed, qcut
        self.nuc_seqs = Counter()
        self._source = None

    def add_nuc_read(self, offset_sequence, count):
        """A read already padded with '-' to its consensus offset."""
        self.nuc_seqs[offset_sequence] += count

    def _attach(self, ctx, slot, g):
        """The reads of this run are run g of the device table `slot`."""
        self._source = (ctx, slot, g)

    def _source_of(self):
        """(ctx, slot, group) of the reads to count insertions over."""
        if self._source is not None:
            return self._source
        if not self.nuc_seqs:
            return None
        reads = list(self.nuc_seqs)
        ctx = session.context()
        ctx.a2c_load_rows(SLOT_INSERTS, reads, [0] * len(reads),
                          [self.nuc_seqs[r] for r in reads], [0, len(reads)], _CODON_CHARS)
        return ctx, SLOT_INSERTS, 0

    def write(self, inserts, region, reading_frame=0, report_aminos=()):
        """Rows for each run of inserted consensus codons: the 1-based left
        codon, each amino-acid string with its count, and the coordinate
        position the run precedes.  Runs placed before coordinate position 1
        or past the end are skipped when report_aminos is given.  The strings
        are counted and the rows formatted by the library (mh_a2c_inserts,
        mh_a2c_insert_rows)."""
        if len(inserts) == 0:
            return
        before = {}
        for ra in report_aminos:
            before.setdefault(ra.seed_amino.consensus_index, ra.position)
        target = {}
        for left, right in _ranges(inserts):
            if right in before:
                target[left] = before[right]
        kept = [r for r in _ranges(inserts)
                if not report_aminos or target.get(r[0]) not in (1, None)]
        if not kept:
            return
        source = self._source_of()
        if source is None:
            return
        # the leading text columns go through the csv module (quoting); the
        # rest are numbers and amino-acid letters, which never need quotes
        lead = io.StringIO()
        csv.writer(lead, lineterminator='').writerow([self.seed, region, self.qcut, ''])
        ctx, slot, g = source
        lefts, rights = [r[0] for r in kept], [r[1] for r in kept]
        targets = [target.get(r[0]) for r in kept]
        if _SHARD is not None and slot == SLOT_REPORT:
            # every rank's strings over its own rows, added up (the first
            # rows are the job's row numbers within the group)
            from .sharded_io import _checked
            mine = _checked(_SHARD, lambda: ctx.a2c_inserts_local(slot, g, reading_frame, lefts, rights))
            text = ctx.a2c_inserts_merged_text(slot, b''.join(_SHARD.all_gather_bytes(mine)), lefts,
                                               lead.getvalue(), targets, os.linesep)
        else:
            text = ctx.a2c_inserts_text(slot, g, reading_frame, lefts, rights, lead.getvalue(), targets,
                                        os.linesep)
        if text:
            self._file.write(text)


def format_cutoff(cutoff):
    """Name of a mixture cutoff in conseq.csv: 'MAX' or three decimals."""
    return cutoff if cutoff == MAX_CUTOFF else '%.3f' % cutoff


SHARD_STATS = {}   # how the last sharded call ran (tests): rows and bytes this rank parsed
_SHARD = None      # the job's Shard while a sharded aln2counts runs (InsertionWriter.write)


def aln2counts(aligned_csv, nuc_csv, amino_csv, coord_ins_csv, conseq_csv,
               failed_align_csv=None, nuc_variants_csv=None, callback=None,
               coverage_summary_csv=None, json=None, variants_csv=None, clipping_csv=None,
               nuc_detail_csv=None, conseq_ins_csv=None, amino_detail_csv=None, linkage_csv=None,
               linkage_positions=None, linkage_min_count=1, concordance_csv=None, covariation_csv=None,
               covariation_min_fraction=0.01, covariation_min_count=10,
               covariation_max_variants=COVARIATION_MAX_VARIANTS, strand_csv=None):
    """aligned.csv -> nucleotide, amino-acid, insertion, consensus (and the
    optional failure, variant and coverage) reports; every argument is an
    open file except json, a project-file path (None: the default).
    variants_csv takes the top nucleotide variants of every coordinate region
    (SequenceReport.write_variants); nuc_variants_csv fails as the
    reference's does.  nuc_detail_csv takes nuc.csv's rows with the N,
    deletion, soft-clip and coverage counts (SequenceReport.write_nuc_detail);
    clipping_csv is the input its clip column comes from, sam2aln's
    clipping.csv (None: the column stays empty).  conseq_ins_csv is an input
    too, sam2aln's conseq_ins.csv: with it nuc_detail_csv's rows end with an
    ins column, the units that carry an insertion after the position.
    concordance_csv is an input as well, sam2aln's concordance.csv: with it
    nuc_detail_csv's rows end with overlap, mismatch and indel, the pairs
    whose mates both align the position and those that disagree there.
    strand_csv is an input too, sam2aln's strand.csv: with it nuc_detail_csv's
    rows end with A_fwd, A_rev, ... del_fwd, del_rev, the units whose mate on
    that strand supports the base at the position and the row's q-cutoff.
    amino_detail_csv takes amino.csv's rows with the X, partial, del, ins, clip
    and coverage columns (SequenceReport.write_amino_detail): the codons read
    at the position that amino.csv leaves out, counted on the device only
    when this is asked for; its ins and clip columns come from the same two
    inputs (read once for both detail files) and stay empty without them.
    linkage_csv takes the amino acids single reads link at the positions of
    linkage_positions (SequenceReport.count_linkage): {coordinate region:
    [set of 1-based positions, ...]}, or the path of a JSON file holding only
    that mapping; haplotypes counted fewer than linkage_min_count times are
    left out (their rows still count in coverage).  A bad set raises
    ValueError before any device work; linkage_positions without linkage_csv
    does nothing.
    covariation_csv takes, for every pair of the minority variants each run's
    own counts select (SequenceReport.count_covariation), how often single
    reads carry one, the other and both; covariation_min_fraction and
    covariation_min_count select the variants (and min_count the pairs),
    covariation_max_variants (at most 256) caps them.  A threshold out of
    range raises ValueError before any device work.

    In a sharded job the counting is split: every rank counts the rows in
    its share of aligned.csv and the ranks add their counters up
    (_load_sharded); every rank then builds the same reports from the
    job's counters, and rank 0 writes them (session.writer_stage).  The
    insertion strings are counted the same way (InsertionWriter.write).
    When aligned.csv cannot be split (not a plain file on every rank, '\r'
    or quoted fields), rank 0 computes alone while the others wait; so it
    does when any rank was given variants_csv (the variants are counted over
    all rows of a run at once, not merged across ranks).  When any rank was
    given amino_detail_csv every rank counts the codon classes of its own rows
    and the tables are added up.  When any rank was given linkage_csv every
    rank counts rank 0's sets over its own rows and the entries are added up
    by (set, haplotype); with variants_csv as well the whole call is
    unsplit.  When any rank was given covariation_csv the variants are
    selected from the job's tables (the codon classes are added up for it)
    with rank 0's thresholds, every rank computes the matrix of its own rows
    and the matrices are added."""
    global _SHARD
    covar = _check_covariation(covariation_min_fraction, covariation_min_count, covariation_max_variants)
    if covariation_csv is None:
        covar = None
    link = None                 # (sets, min_count) when linkage.csv is asked for
    if linkage_csv is not None:
        if linkage_positions is None:
            raise ValueError('linkage: linkage_csv needs linkage_positions')
        link = _check_linkage(_load_linkage(linkage_positions), linkage_min_count), linkage_min_count
    sh = session.shard()
    SHARD_STATS.clear()
    session.stats['aln2counts_source'] = 'csv'
    handles = (nuc_csv, amino_csv, coord_ins_csv, conseq_csv, failed_align_csv, nuc_variants_csv,
               coverage_summary_csv, variants_csv, nuc_detail_csv, amino_detail_csv, linkage_csv,
               covariation_csv)
    with session.writer_stage(*handles) as stage:
        split = sh is not None
        if split:
            from .sharded_io import _agree_ok
            if not _agree_ok(sh, variants_csv is None):    # asked for on some rank
                split = False
                SHARD_STATS.update(mode='unsplit', reason='variants_csv')
        # asked for on some rank: then every rank enters the sum of the tables
        job_detail = split and not _agree_ok(sh, amino_detail_csv is None)
        job_link = None
        if split and not _agree_ok(sh, linkage_csv is None):
            # the sets are rank 0's, so that every rank enters the same collectives
            spec = sh.all_gather_bytes(jsonlib.dumps(link).encode() if link else b'')[0]
            job_link = tuple(jsonlib.loads(spec.decode())) if spec else None
        job_covar = None
        if split and not _agree_ok(sh, covariation_csv is None):
            # rank 0's thresholds, and the job's del counts to select with
            spec = sh.all_gather_bytes(jsonlib.dumps(covar).encode() if covar else b'')[0]
            job_covar = tuple(jsonlib.loads(spec.decode())) if spec else None
            job_detail = job_detail or job_covar is not None
        groups = _load_sharded(sh, aligned_csv) if split else None
        if groups is None:
            if stage.active:
                _aln2counts(aligned_csv, nuc_csv, amino_csv, coord_ins_csv, conseq_csv,
                            failed_align_csv, nuc_variants_csv, callback, coverage_summary_csv, json,
                            variants_csv=variants_csv, clipping_csv=clipping_csv,
                            nuc_detail_csv=nuc_detail_csv, conseq_ins_csv=conseq_ins_csv,
                            amino_detail_csv=amino_detail_csv, linkage_csv=linkage_csv, link=link,
                            concordance_csv=concordance_csv, covariation_csv=covariation_csv, covar=covar,
                            strand_csv=strand_csv)
            return
        # every rank builds the reports; the others' go nowhere
        outs = handles if stage.active else tuple(None if h is None else io.StringIO() for h in handles)
        _SHARD = sh
        try:
            _aln2counts(aligned_csv, outs[0], outs[1], outs[2], outs[3], outs[4], outs[5],
                        callback if stage.active else None, outs[6], json, groups=groups,
                        clipping_csv=clipping_csv, nuc_detail_csv=outs[8],
                        conseq_ins_csv=conseq_ins_csv, amino_detail_csv=outs[9], job_detail=job_detail,
                        linkage_csv=None if job_link is None else outs[10] or io.StringIO(), link=job_link,
                        concordance_csv=concordance_csv,
                        covariation_csv=None if job_covar is None else outs[11] or io.StringIO(),
                        covar=job_covar, strand_csv=strand_csv)
        finally:
            _SHARD = None


def _load_sharded(sh, aligned_csv):
    """This rank's share of aligned.csv counted into the job's groups, the
    counters added up over the ranks: the number of (refname, qcut) groups,
    or None (on every rank) when the file is not split."""
    from .sharded_io import _agree_ok, _checked
    ctx = session.context()
    fd = session.readable_fd(aligned_csv)
    if not _agree_ok(sh, fd is not None):
        return None
    part = _checked(sh, lambda: ctx.a2c_part_open(SLOT_REPORT, fd, sh.rank, sh.world, _CODON_CHARS))
    if not _agree_ok(sh, part is not None):
        return None
    aligned_csv.seek(0, 2)    # consumed, as the reference's DictReader leaves it
    keys, rows, ncod, total = ctx.a2c_part_groups(SLOT_REPORT, part['groups'])
    all_keys = sh.all_gather_bytes(keys)
    all_meta = sh.all_gather_bytes(np.concatenate([rows, ncod.reshape(-1), total]).astype(np.int64).tobytes())
    # the job's groups: runs of equal keys in rank order (a run can go on
    # across the ranks' cuts)
    g_keys, g_ncod, g_total, g_rows = [], [], [], []
    mine_gid, mine_base = [], []
    for r in range(sh.world):
        ks = all_keys[r].split(b'\n')[:-1] if all_keys[r] else []
        meta = np.frombuffer(all_meta[r], dtype=np.int64)
        n = len(ks)
        rr, nc, tt = meta[:n], meta[n:4 * n].reshape(n, 3), meta[4 * n:5 * n]
        for k in range(n):
            if k == 0 and g_keys and g_keys[-1] == ks[k]:
                g = len(g_keys) - 1
                g_ncod[g] = np.maximum(g_ncod[g], nc[k])
            else:
                g = len(g_keys)
                g_keys.append(ks[k])
                g_ncod.append(nc[k].copy())
                g_total.append(0)
                g_rows.append(0)
            if r == sh.rank:
                mine_gid.append(g)
                mine_base.append(g_rows[g])
            g_total[g] += int(tt[k])
            g_rows[g] += int(rr[k])
    for g, t in enumerate(g_total):
        if t > 0xffffffff:
            raise _native.NativeError('aln2counts: the counts of group %d add up to more than 2**32-1' % g)
    cells = ctx.a2c_part_count(SLOT_REPORT, b''.join(k + b'\n' for k in g_keys), mine_gid,
                               np.array(g_ncod, dtype=np.int32).reshape(-1, 3), mine_base)
    cnt, first = ctx.a2c_part_counters(SLOT_REPORT, cells)
    total_cnt = sh.sum_i64(cnt.astype(np.int64))
    first64 = np.where(first == np.uint32(0xffffffff), -1, first.astype(np.int64))
    least = sh.min_i64(first64)
    ctx.a2c_part_counters(SLOT_REPORT, cells, (total_cnt.astype(np.uint32),
                                               np.where(least < 0, 0xffffffff, least).astype(np.uint32)))
    SHARD_STATS.update(mode='sharded', rows=part['rows'], bytes=part['bytes'])
    return len(g_keys)


def _aln2counts(aligned_csv, nuc_csv, amino_csv, coord_ins_csv, conseq_csv, failed_align_csv,
                nuc_variants_csv, callback, coverage_summary_csv, json, groups=None,
                variants_csv=None, clipping_csv=None, nuc_detail_csv=None, conseq_ins_csv=None,
                amino_detail_csv=None, job_detail=False, linkage_csv=None, link=None,
                concordance_csv=None, covariation_csv=None, covar=None, strand_csv=None):
    projects = (project_config.ProjectConfig.loadDefault() if json is None
                else project_config.ProjectConfig.loadCustom(json))
    report = SequenceReport(InsertionWriter(coord_ins_csv), projects, CONSEQ_MIXTURE_CUTOFFS)
    report.write_nuc_header(nuc_csv)
    report.write_amino_header(amino_csv)
    report.write_consensus_header(conseq_csv)
    # what is written for each run, in the reference's file order
    per_run = [lambda: report.write_amino_counts(amino_csv, coverage_summary=summary),
               lambda: report.write_consensus(conseq_csv)]
    if failed_align_csv:
        report.write_failure_header(failed_align_csv)
        per_run.append(lambda: report.write_failure(failed_align_csv))
    per_run += [report.write_insertions, lambda: report.write_nuc_counts(nuc_csv)]
    if nuc_variants_csv:
        report.write_nuc_variants_header(nuc_variants_csv)
        per_run.append(lambda: report.write_nuc_variants(nuc_variants_csv))
    if variants_csv is not None:
        report.write_nuc_variants_header(variants_csv)
        per_run.append(lambda: report.write_variants(variants_csv))
    if nuc_detail_csv is not None or amino_detail_csv is not None:
        clipping = None if clipping_csv is None else _read_clipping(clipping_csv)
        insertions = None if conseq_ins_csv is None else _read_conseq_ins(conseq_ins_csv)
    if nuc_detail_csv is not None:
        concordance = None if concordance_csv is None else _read_concordance(concordance_csv)
        strand = None if strand_csv is None else _read_strand(strand_csv)
        report.write_nuc_detail_header(nuc_detail_csv, insertions is not None, concordance is not None,
                                       strand is not None)
        per_run.append(lambda: report.write_nuc_detail(nuc_detail_csv, clipping, insertions, concordance,
                                                       strand))
    if amino_detail_csv is not None:
        report.write_amino_detail_header(amino_detail_csv)
        per_run.append(lambda: report.write_amino_detail(amino_detail_csv, clipping, insertions))
    if linkage_csv is not None:
        report.write_linkage_header(linkage_csv)
        per_run.append(lambda: report.write_linkage(linkage_csv, *link))
    if covariation_csv is not None:
        report.write_covariation_header(covariation_csv)
        per_run.append(lambda: report.write_covariation(covariation_csv, *covar))
    summary = None
    if coverage_summary_csv is not None:
        summary_writer = _csv_writer(coverage_summary_csv, 'coverage')
        summary_writer.writeheader()
        summary = {}
    source = getattr(aligned_csv, 'name', None) if callback else None
    if source:
        report.enable_callback(callback, os.stat(source).st_size)
    ctx = session.context()
    session.stats['aln2counts_source'] = 'csv'
    if groups is None:           # not loaded by the ranks of a sharded job
        if (os.environ.get('MICALL_ALN2COUNTS_RESIDENT', '1') != '0' and
                session.aligned_resident(ctx, aligned_csv)):
            # the file this process's sam2aln() just wrote: its rows are on
            # the device already (None: they cannot stand for the file)
            groups = ctx.a2c_load_resident(SLOT_REPORT, _CODON_CHARS)
            if groups is not None:
                aligned_csv.seek(0, 2)
                session.stats['aln2counts_source'] = 'device'
        fd = session.readable_fd(aligned_csv) if groups is None else None
        if fd is not None:   # the file mmap'd by the library (no '\r' in it)
            groups = ctx.a2c_load_file(SLOT_REPORT, fd, _CODON_CHARS)
            if groups is not None:
                aligned_csv.seek(0, 2)
        if groups is None:
            groups = ctx.a2c_load_csv(SLOT_REPORT, session.read_text(aligned_csv), _CODON_CHARS)
    tables = _job_detail(ctx, groups) if job_detail else None
    for g in range(groups):
        report._read_group(ctx, SLOT_REPORT, g)
        if tables is not None:
            report._job_detail = tables[g]
        for step in per_run:
            step()
    if summary:
        summary_writer.writerow(summary)


def _job_detail(ctx, groups):
    """Per group the three frames' (codons, 3) X / partial / del tables of a
    sharded job: every rank's counts of its own rows (mh_a2c_codon_detail
    after mh_a2c_part_count), added up over the ranks in one collective that
    every rank enters."""
    from .sharded_io import _checked
    ncod = [ctx.a2c_group(SLOT_REPORT, g)['ncod'] for g in range(groups)]
    mine = _checked(_SHARD, lambda: [ctx.a2c_codon_detail(SLOT_REPORT, g, f, ncod[g][f]).astype(np.int64)
                                     for g in range(groups) for f in range(3)])
    total = _SHARD.sum_i64(np.concatenate([t.reshape(-1) for t in mine] + [np.zeros(1, np.int64)]))
    tables, at = [], 0
    for g in range(groups):
        tables.append([])
        for f in range(3):
            tables[g].append(total[at:at + 3 * ncod[g][f]].reshape(-1, 3))
            at += 3 * ncod[g][f]
    return tables


def _read_clipping(clipping_csv):
    """{refname: {pos: count}} of sam2aln's clipping.csv."""
    clipping = {}
    for row in csv.DictReader(clipping_csv):
        clipping.setdefault(row['refname'], {})[int(row['pos'])] = int(row['count'])
    return clipping


_NO_STRAND = (0,) * 10


def _read_strand(strand_csv):
    """{refname: {(qcut, pos): (A_fwd, A_rev, C_fwd, ... del_fwd, del_rev)}} of sam2aln's strand.csv."""
    strand = {}
    for row in csv.DictReader(strand_csv):
        strand.setdefault(row['refname'], {})[int(row['qcut']), int(row['pos'])] = tuple(
            int(row[k]) for k in _SCHEMA['nuc_detail_strand'])
    return strand


def _read_concordance(concordance_csv):
    """{refname: {pos: (overlap, mismatch, indel)}} of sam2aln's concordance.csv."""
    concordance = {}
    for row in csv.DictReader(concordance_csv):
        concordance.setdefault(row['refname'], {})[int(row['pos'])] = (
            int(row['overlap']), int(row['mismatch']), int(row['indel']))
    return concordance


def _read_conseq_ins(conseq_ins_csv):
    """{refname: {(qcut, pos): count summed over the strings}} of sam2aln's
    conseq_ins.csv."""
    insertions = {}
    for row in csv.DictReader(conseq_ins_csv):
        per_ref = insertions.setdefault(row['refname'], {})
        key = int(row['qcut']), int(row['pos'])
        per_ref[key] = per_ref.get(key, 0) + int(row['count'])
    return insertions


def _arguments(argv=None):
    cli = argparse.ArgumentParser(description='aln2counts on the MI355X: counts, consensus and '
                                              'insertions from aligned.csv.')
    cli.add_argument('aligned_csv', type=argparse.FileType('r'), help='aligned.csv from sam2aln')
    for name, what in (('nuc_csv', 'nucleotide counts'), ('amino_csv', 'amino-acid counts'),
                       ('coord_ins_csv', 'insertions in coordinate positions'),
                       ('conseq_csv', 'consensus sequences')):
        cli.add_argument(name, type=argparse.FileType('w'), help='output: ' + what)
    cli.add_argument('--failed_align_csv', type=argparse.FileType('w'),
                     help='output: consensus sequences that did not align')
    cli.add_argument('--nuc_variants_csv', type=argparse.FileType('w'),
                     help='output: nucleotide variants')
    cli.add_argument('--variants_csv', type=argparse.FileType('w'),
                     help='output: top nucleotide variants of every coordinate region')
    cli.add_argument('--clipping_csv', type=argparse.FileType('r'),
                     help="input: sam2aln's clipping.csv, for the clip column of the detail files")
    cli.add_argument('--conseq_ins_csv', type=argparse.FileType('r'),
                     help="input: sam2aln's conseq_ins.csv, for the ins column of the detail files")
    cli.add_argument('--concordance_csv', type=argparse.FileType('r'),
                     help="input: sam2aln's concordance.csv, for the overlap, mismatch and indel "
                          "columns of nuc_detail_csv")
    cli.add_argument('--strand_csv', type=argparse.FileType('r'),
                     help="input: sam2aln's strand.csv, for the ten fwd and rev columns of nuc_detail_csv")
    cli.add_argument('--nuc_detail_csv', type=argparse.FileType('w'),
                     help='output: nuc.csv with N, deletion, soft-clip and coverage counts')
    cli.add_argument('--amino_detail_csv', type=argparse.FileType('w'),
                     help='output: amino.csv with X, partial, del, ins, clip and coverage counts')
    cli.add_argument('--linkage_csv', type=argparse.FileType('w'),
                     help='output: amino acids linked by single reads at the positions of --linkage_positions')
    cli.add_argument('--linkage_positions', metavar='FILE.json',
                     help='input: {coordinate region: [[1-based amino-acid positions], ...]} as JSON')
    cli.add_argument('--linkage_min_count', type=int, default=1, metavar='N',
                     help='leave out linked haplotypes counted fewer than N times (default 1)')
    cli.add_argument('--covariation_csv', type=argparse.FileType('w'),
                     help='output: which minority variants single reads carry together, pair by pair')
    cli.add_argument('--covariation_min_fraction', type=float, default=0.01, metavar='F',
                     help="a variant is read in at least F of its position's called reads (default 0.01)")
    cli.add_argument('--covariation_min_count', type=int, default=10, metavar='N',
                     help='a variant, and the reads called at both positions of a pair, count at least N '
                          '(default 10)')
    cli.add_argument('--covariation_max_variants', type=int, default=COVARIATION_MAX_VARIANTS, metavar='N',
                     help='keep the N most counted variants of a run (default and most: 256)')
    return cli.parse_args(argv)


parseArgs = _arguments


def main():
    a = _arguments()
    aln2counts(a.aligned_csv, a.nuc_csv, a.amino_csv, a.coord_ins_csv, a.conseq_csv,
               a.failed_align_csv, a.nuc_variants_csv, variants_csv=a.variants_csv,
               clipping_csv=a.clipping_csv, nuc_detail_csv=a.nuc_detail_csv,
               conseq_ins_csv=a.conseq_ins_csv, amino_detail_csv=a.amino_detail_csv,
               linkage_csv=a.linkage_csv, linkage_positions=a.linkage_positions,
               linkage_min_count=a.linkage_min_count, concordance_csv=a.concordance_csv,
               covariation_csv=a.covariation_csv, covariation_min_fraction=a.covariation_min_fraction,
               covariation_min_count=a.covariation_min_count,
               covariation_max_variants=a.covariation_max_variants, strand_csv=a.strand_csv)


if __name__ == '__main__':
    main()
