"""
Drop-in for micall/core/sam2aln.py: same function, arguments and output files.

sam2aln() reads remap.csv, pairs rows by qname, merges each pair into one
sequence in consensus coordinates (apply_cigar, then merge_pairs at each of
SAM2ALN_Q_CUTOFFS, all in one device pass), drops pairs with more than half
of their bases censored, and writes the
distinct merged sequences with their counts per reference (aligned.csv), the
insertions the merge removed (insert.csv) and the pairs that failed
(failed.csv) -- sam2aln.py:395-478.  The per-pair work and the count of
identical sequences run on the device (mh_sam2aln_csv, mh_sam2aln.hip); the
host parses the CSV and writes the text.  nthreads is accepted for signature
compatibility and ignored.  There is no CPU fallback.

When remap_csv is the unchanged file this process's remap() just wrote from
records that are still resident (session.remap_resident), nothing is parsed:
the rows are built on the device from the resident reads and records
(mh_sam2aln_resident) and the outputs are the same bytes.
session.stats['sam2aln_source'] says which way a call went ('device' or
'csv'); MICALL_SAM2ALN_RESIDENT=0 in the environment forces the file path.

The aligned.csv a call wrote is recorded (session.aligned_written) when it
is exactly the text the library formatted, so that aln2counts() in the same
process can count the rows where they are instead of parsing the file.

In a sharded job (torchrun) every rank takes its share of remap.csv's rows,
merges its pairs on its GPU, and writes its own insert.csv / failed.csv rows
and its piece of aligned.csv at all-gathered offsets; the distinct merged
sequences are counted by hash owner and sorted across the ranks by a sample
sort (_sam2aln_sharded, mh_s2a_shard.cpp) -- the reference's own pool splits
parse_sam over pairs the same way (sam2aln.py:411-424).  The split takes one
q-cutoff; with more, rank 0 does the whole stage.

clipping_csv (optional, not in the reference): per consensus position the
number of merged units that soft-clip it while no mate aligns it
(refname,pos,count), counted on the device from the rows the merge left
there (mh_sam2aln_clipping: k_s2a_clip, k_s2a_clip_scan) on every route.
A call without it launches and allocates nothing for it.

conseq_ins_csv (optional, not in the reference): the insertions that the
last remap pass left out of the consensus -- apply_cigar takes them out of
the read and aligned.csv has no trace of them -- merged per unit and
q-cutoff as the reference's merge_inserts merges them (sam2aln.py:240-273)
and counted per distinct string: refname,qcut,pos,insert,count, pos the
consensus position the insertion follows (not insert.csv's read-derived
pos).  Counted on the device like the clipping (mh_sam2aln_conseq_ins:
k_s2a_ins_rec, k_s2a_ins_merge, k_s2a_ins_tab), only when asked for.

concordance_csv and cycle_concordance_csv (optional, not in the reference):
what the merge sees and drops.  Over the paired units that reach the merge,
whatever the q-cutoffs: per consensus position both mates align, the units
(overlap) and those whose mates disagree there (mismatch, indel, nocall,
and unresolved: qualities closer than 5, an N at every cutoff); and per
read (1, 2) and sequencing cycle or reported quality, the bases compared
with the mate's and found different -- the sample's own error estimate,
with no phiX.  A cycle is the base's place in the read as the FASTQ held
it, so after trim_fastqs it counts from the trimmed 5' end.  Counted on
the device like the clipping (mh_sam2aln_concordance: k_s2a_conc,
k_s2a_conc_scan), once for both files and only when asked for.

strand_csv (optional, not in the reference): which strand saw each merged
base.  A unit counts at the cutoffs at which it gives aligned.csv a sequence.
At position y with merged base m (A, C, G, T or '-'), a mate supports m
when its own expansion holds m at y, whatever its quality; the unit adds 1
to m_fwd when a supporting mate is forward (FLAG 0x10 clear), 1 to m_rev
when one is reversed, and 1 to m_both when both hold: refname,qcut,pos and
the fifteen counts, so that fwd + rev - both is the number of aligned.csv's
sequences (by count) that hold m there.  Counted on the device like the
clipping (mh_sam2aln_strand: k_s2a_strand, k_s2a_strand_scan), once for all
the cutoffs and only when asked for.
"""
import argparse
import os

import numpy as np

from . import session

SAM2ALN_Q_CUTOFFS = [15]  # sam2aln.py:24
MAX_PROP_N = 0.5          # sam2aln.py:25
MAX_Q_CUTOFFS = 8         # distinct cutoffs of one device pass (mh_sam2aln_csv_q)


SHARD_STATS = {}   # how the last sharded call ran (tests): mode, rows parsed


def _cutoff_list(q_cutoffs):
    """The distinct cutoffs in first-seen order: the reference keeps one
    merged sequence per cutoff in a dict (mseqs[qcut], sam2aln.py:402), so a
    repeated cutoff changes nothing."""
    cuts = []
    for q in SAM2ALN_Q_CUTOFFS if q_cutoffs is None else q_cutoffs:
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)):
            raise ValueError('q-cutoff {!r} is not an integer'.format(q))
        if int(q) not in cuts:
            cuts.append(int(q))
    if not 1 <= len(cuts) <= MAX_Q_CUTOFFS:
        raise ValueError('{} distinct q-cutoffs: the device merge takes 1 to {}'.format(
            len(cuts), MAX_Q_CUTOFFS))
    return cuts


def sam2aln(remap_csv, aligned_csv, insert_csv=None, failed_csv=None, nthreads=None, q_cutoffs=None,
            clipping_csv=None, conseq_ins_csv=None, concordance_csv=None, cycle_concordance_csv=None,
            strand_csv=None):
    """sam2aln.sam2aln (sam2aln.py:395-478).  q_cutoffs: the list of quality
    cutoffs, None for the module's SAM2ALN_Q_CUTOFFS (where the reference's
    users set it).  In a sharded job every rank does its share
    (_sam2aln_sharded); when remap.csv cannot be split that way, rank 0
    computes and writes while the other ranks wait (session.writer_stage).
    clipping_csv: an open file for the soft-clip counts, None for none;
    conseq_ins_csv: one for the merged insertions; concordance_csv and
    cycle_concordance_csv: one each for the mates' concordance per consensus
    position and per read cycle and quality; strand_csv: one for the strand
    support of every merged base."""
    cuts = _cutoff_list(q_cutoffs)
    sh = session.shard()
    SHARD_STATS.clear()
    session.stats['sam2aln_source'] = 'csv'
    session.aligned_forget()     # recorded again below, once aligned.csv is these results
    use_resident = os.environ.get('MICALL_SAM2ALN_RESIDENT', '1') != '0'
    if sh is not None and _sam2aln_sharded(sh, remap_csv, aligned_csv, insert_csv, failed_csv, cuts,
                                           clipping_csv, conseq_ins_csv, concordance_csv,
                                           cycle_concordance_csv, strand_csv):
        return
    with session.writer_stage(aligned_csv, insert_csv, failed_csv, clipping_csv,
                              conseq_ins_csv, concordance_csv, cycle_concordance_csv,
                              strand_csv) as stage:
        if not stage.active:
            return
        ctx = session.context()
        done = None
        if use_resident and session.remap_resident(ctx, remap_csv):
            done = ctx.sam2aln_resident(session.remap_refnames(), q_cutoffs=cuts, max_prop_n=MAX_PROP_N)
            if done is not None:
                remap_csv.seek(0, 2)     # consumed, as below
                session.stats['sam2aln_source'] = 'device'
        fd = session.readable_fd(remap_csv) if done is None else None
        if fd is not None:   # the file mmap'd by the library (no '\r' in it)
            done = ctx.sam2aln_file(fd, q_cutoffs=cuts, max_prop_n=MAX_PROP_N)
            if done is not None:
                remap_csv.seek(0, 2)     # consumed, as the reference's DictReader leaves it
        if done is None:
            text = session.read_text(remap_csv)
            ctx.sam2aln_csv(text, q_cutoffs=cuts, max_prop_n=MAX_PROP_N)
        if clipping_csv:
            _write_side(clipping_csv, ctx.sam2aln_clipping_write, ctx.sam2aln_clipping)
        if conseq_ins_csv:
            _write_side(conseq_ins_csv, ctx.sam2aln_conseq_ins_write, ctx.sam2aln_conseq_ins)
        for which, handle in enumerate((concordance_csv, cycle_concordance_csv)):
            if handle:
                _write_side(handle, lambda fd, at, w=which: ctx.sam2aln_concordance_write(w, fd, at),
                            lambda w=which: ctx.sam2aln_concordance(w))
        if strand_csv:
            _write_side(strand_csv, ctx.sam2aln_strand_write, ctx.sam2aln_strand)
        for which, handle in (('insert', insert_csv), ('failed', failed_csv), ('aligned', aligned_csv)):
            if handle:
                start = _write_output(ctx, which, handle)
                if which == 'aligned':
                    _record_aligned(ctx, handle, start, sh)


SAMPLES_PER_NAME = 64   # sample records per reference and rank for the splitters


def _sam2aln_sharded(sh, remap_csv, aligned_csv, insert_csv, failed_csv, cuts=None, clipping_csv=None,
                     conseq_ins_csv=None, concordance_csv=None, cycle_concordance_csv=None,
                     strand_csv=None):
    """This rank's share of sam2aln.  False (on every rank, before any
    output is written) when the job must fall back to rank 0 alone: more
    than one q-cutoff (every rank holds the same list, so none has to ask),
    a remap.csv that is not a plain file on every rank, one with quoted
    fields or '\r', or a qname whose rows sit on two ranks."""
    if cuts is None:
        cuts = _cutoff_list(None)
    if len(cuts) != 1:
        return False
    from . import sharded_io
    from .sharded_io import SharedOutput, _agree_ok, _checked
    ctx = session.context()
    fd = session.readable_fd(remap_csv)
    if not _agree_ok(sh, fd is not None):
        return False
    sh.barrier()             # every rank opened (truncated) the outputs
    part = _checked(sh, lambda: ctx.sam2aln_part(fd, sh.rank, sh.world, cuts[0],
                                                  MAX_PROP_N))
    if not _agree_ok(sh, part is not None):
        return False
    hashes, leftover = ctx.sam2aln_part_units(part['units'])
    if sharded_io.qname_conflict(sh, hashes, leftover):
        return False
    remap_csv.seek(0, 2)     # consumed, as the reference's DictReader leaves it
    SHARD_STATS.update(mode='sharded', bytes=part['bytes'], file_bytes=part['file_bytes'],
                       units=part['units'])
    # reference names in the reference's first-seen order over the job's
    # units: every rank's pair units in rank order, then every rank's leftovers
    names, first = ctx.sam2aln_part_names(part['names'])
    if clipping_csv:
        _clipping_sharded(sh, ctx, names, clipping_csv)
    if conseq_ins_csv:
        _conseq_ins_sharded(sh, ctx, cuts, conseq_ins_csv)
    if concordance_csv or cycle_concordance_csv:
        _concordance_sharded(sh, ctx, names, concordance_csv, cycle_concordance_csv)
    if strand_csv:
        _strand_sharded(sh, ctx, names, cuts, strand_csv)
    texts = sh.all_gather_bytes('\n'.join(names).encode())
    firsts = sh.all_gather_bytes(np.asarray(first, dtype=np.int64).tobytes())
    pairs = sh._gather_sizes([part['pair_units']])[:, 0]
    key = {}
    for r in range(sh.world):
        rn = texts[r].decode().split('\n') if texts[r] else []
        fu = np.frombuffer(firsts[r], dtype=np.int64)
        for n, u in zip(rn, fu.tolist()):
            k = (0, r, u) if u < pairs[r] else (1, r, u)
            if n not in key or k < key[n]:
                key[n] = k
    order = sorted(key, key=key.get)
    gid = {n: i for i, n in enumerate(order)}
    ctx.sam2aln_part_set_names([gid[n] for n in names])
    # aligned.csv: distinct sequences counted by their owner, then sorted
    # across the ranks (sample sort) and written piece by piece
    data, sizes = ctx.sam2aln_records(0, sh.world)
    got = sharded_io.all_to_all_bytes(sh, data, sizes)
    ctx.sam2aln_records_merge(0, got)
    del got
    samples, _ = ctx.sam2aln_records(1, sh.world, SAMPLES_PER_NAME)
    ctx.sam2aln_splitters(np.frombuffer(b''.join(sh.all_gather_bytes(samples.tobytes())), dtype=np.uint8),
                          sh.world)
    data, sizes = ctx.sam2aln_records(2, sh.world)
    got = sharded_io.all_to_all_bytes(sh, data, sizes)
    ctx.sam2aln_records_merge(1, got)
    del got
    counts = sh._gather_sizes(ctx.sam2aln_range_counts(len(order)))     # [rank, name]
    base = counts[:sh.rank].sum(axis=0)
    rows, seg = ctx.sam2aln_range_text(order, base)
    head = b'refname,qcut,rank,count,offset,seq\n' if sh.rank == 0 else b''
    pieces, at = [head], 0
    for n in seg.tolist():
        pieces.append(rows[at:at + n])
        at += n
    out = SharedOutput(sh, aligned_csv)
    out.write_bytes(pieces)
    del rows
    for which, handle in (('insert', insert_csv), ('failed', failed_csv)):
        if handle:
            segs = [ctx.sam2aln_part_text(which, 0, head=sh.rank == 0), ctx.sam2aln_part_text(which, 1)]
            o = SharedOutput(sh, handle)
            o.write_bytes(segs)
            o.finish()
    out.finish()
    sh.barrier()             # every rank's rows are in the files
    for h in (aligned_csv, insert_csv, failed_csv, clipping_csv, conseq_ins_csv, concordance_csv,
              cycle_concordance_csv, strand_csv):
        if h and sh.rank == 0:
            h.flush()
    return True


def _clipping_sharded(sh, ctx, names, clipping_csv):
    """clipping.csv of a sharded call: every rank counts the units of its
    own rows on its device, the (name, pos, count) lists are all-gathered,
    and rank 0 sums them and writes (the barrier at the end of the stage
    holds the other ranks until it has)."""
    import csv
    ids, pos, cnt = ctx.sam2aln_clip_counts()
    mine = '\n'.join(names).encode(), ids.tobytes(), pos.tobytes(), cnt.tobytes()
    parts = [sh.all_gather_bytes(x) for x in mine]
    if sh.rank != 0:
        return
    total = {}
    for r in range(sh.world):
        rn = parts[0][r].decode().split('\n') if parts[0][r] else []
        for i, p, n in zip(np.frombuffer(parts[1][r], dtype=np.int32).tolist(),
                           np.frombuffer(parts[2][r], dtype=np.int64).tolist(),
                           np.frombuffer(parts[3][r], dtype=np.int32).tolist()):
            key = rn[i], p
            total[key] = total.get(key, 0) + n
    w = csv.writer(clipping_csv, lineterminator='\n')
    w.writerow(['refname', 'pos', 'count'])
    w.writerows((name, p, total[name, p]) for name, p in sorted(total))


CONCORDANCE_HEADER = ['refname', 'pos', 'overlap', 'mismatch', 'indel', 'nocall', 'unresolved']
CYCLE_CONCORDANCE_HEADER = ['read', 'by', 'value', 'compared', 'mismatch']


def _concordance_sharded(sh, ctx, names, concordance_csv, cycle_concordance_csv):
    """The two concordance files of a sharded call: every rank counts the
    paired units of its own rows on its device, the position rows and the
    read tables are all-gathered, and rank 0 sums them and writes the files
    that were asked for, as _clipping_sharded does."""
    import csv
    ids, pos, cnt, reads = ctx.sam2aln_conc_counts()
    mine = '\n'.join(names).encode(), ids.tobytes(), pos.tobytes(), cnt.tobytes(), reads.tobytes()
    parts = [sh.all_gather_bytes(x) for x in mine]
    if sh.rank != 0:
        return
    total, table = {}, {}
    for r in range(sh.world):
        rn = parts[0][r].decode().split('\n') if parts[0][r] else []
        for i, p, five in zip(np.frombuffer(parts[1][r], dtype=np.int32).tolist(),
                              np.frombuffer(parts[2][r], dtype=np.int64).tolist(),
                              np.frombuffer(parts[3][r], dtype=np.int32).reshape(-1, 5).tolist()):
            key = rn[i], p
            total[key] = [a + b for a, b in zip(total[key], five)] if key in total else five
        for read, by, value, compared, mismatch in np.frombuffer(parts[4][r],
                                                                 dtype=np.int64).reshape(-1, 5).tolist():
            old = table.get((read, by, value), (0, 0))
            table[read, by, value] = old[0] + compared, old[1] + mismatch
    if concordance_csv:
        w = csv.writer(concordance_csv, lineterminator='\n')
        w.writerow(CONCORDANCE_HEADER)
        w.writerows([name, p] + total[name, p] for name, p in sorted(total))
    if cycle_concordance_csv:
        w = csv.writer(cycle_concordance_csv, lineterminator='\n')
        w.writerow(CYCLE_CONCORDANCE_HEADER)
        w.writerows((read, 'quality' if by else 'cycle', value) + table[read, by, value]
                    for read, by, value in sorted(table))


STRAND_HEADER = ['refname', 'qcut', 'pos'] + [base + strand for base in ('A', 'C', 'G', 'T', 'del')
                                              for strand in ('_fwd', '_rev', '_both')]


def _strand_sharded(sh, ctx, names, cuts, strand_csv):
    """strand.csv of a sharded call: every rank counts its own units on its
    device, the rows are all-gathered, and rank 0 sums them and writes in the
    file's order (names as str sorts, the call's cutoffs, positions), as
    _concordance_sharded does."""
    import csv
    ids, cut, pos, cnt = ctx.sam2aln_strand_counts()
    mine = '\n'.join(names).encode(), ids.tobytes(), cut.tobytes(), pos.tobytes(), cnt.tobytes()
    parts = [sh.all_gather_bytes(x) for x in mine]
    if sh.rank != 0:
        return
    total = {}
    for r in range(sh.world):
        rn = parts[0][r].decode().split('\n') if parts[0][r] else []
        for i, q, p, fifteen in zip(np.frombuffer(parts[1][r], dtype=np.int32).tolist(),
                                    np.frombuffer(parts[2][r], dtype=np.int32).tolist(),
                                    np.frombuffer(parts[3][r], dtype=np.int64).tolist(),
                                    np.frombuffer(parts[4][r], dtype=np.int32).reshape(-1, 15).tolist()):
            key = rn[i], q, p
            total[key] = [a + b for a, b in zip(total[key], fifteen)] if key in total else fifteen
    w = csv.writer(strand_csv, lineterminator='\n')
    w.writerow(STRAND_HEADER)
    w.writerows([name, q, p] + total[name, q, p]
                for name, q, p in sorted(total, key=lambda k: (k[0], cuts.index(k[1]), k[2])))


def _conseq_ins_sharded(sh, ctx, cuts, conseq_ins_csv):
    """conseq_ins.csv of a sharded call (one q-cutoff): every rank counts the
    insertions of its own units on its device, the (name, pos, insert, count)
    lists -- each rank's own conseq_ins.csv rows -- are all-gathered, and
    rank 0 adds them up and writes in the file's order."""
    import csv
    import io
    parts = sh.all_gather_bytes(ctx.sam2aln_conseq_ins().encode())
    if sh.rank != 0:
        return
    total = {}
    for part in parts:
        for row in csv.DictReader(io.StringIO(part.decode())):
            key = row['refname'], int(row['pos']), row['insert']
            total[key] = total.get(key, 0) + int(row['count'])
    w = csv.writer(conseq_ins_csv, lineterminator='\n')
    w.writerow(['refname', 'qcut', 'pos', 'insert', 'count'])
    w.writerows((name, cuts[0], pos, ins, n) for (name, pos, ins), n in
                sorted(total.items(), key=lambda kv: (kv[0][0], kv[0][1], -kv[1], kv[0][2].encode())))


def _write_side(handle, write, text):
    """clipping.csv or conseq_ins.csv, as _write_output writes the other
    three: write(fd, offset) for a plain file, else text() through the handle."""
    from .sharded_io import SharedOutput
    out = SharedOutput(None, handle)
    if out.direct:
        out.end += write(out.fd, int(out.end))
        out.finish()
    else:
        handle.write(text())


def _write_output(ctx, which, handle):
    """One output: written by the library at the handle's position when it is
    a plain file (pwrite), else through the handle.  Returns the file offset
    the library wrote from, None when the text went through the handle."""
    from .sharded_io import SharedOutput
    out = SharedOutput(None, handle)
    if out.direct:
        # formatted and written together (pwrite from the handle's position)
        start = int(out.end)
        out.end += ctx.sam2aln_write(which, out.fd, start)
        out.finish()
        return start
    handle.write(ctx.sam2aln_output(which))
    return None


def _record_aligned(ctx, handle, start, sh):
    """aln2counts() may count the rows on the device instead of parsing
    aligned.csv when the file is exactly what the library just wrote: one
    process, written from offset 0 of a plain file that now ends where the
    write did (session.aligned_resident tests the rest when it is read)."""
    written = ctx.sam2aln_written('aligned') if sh is None and start == 0 else None
    try:
        whole = written is not None and os.fstat(handle.fileno()).st_size == written[1]
    except (AttributeError, OSError, ValueError):
        whole = False
    if whole:
        session.aligned_written(ctx, handle, written)
    else:
        session.aligned_forget()


def parseArgs():
    parser = argparse.ArgumentParser(description='Conversion of SAM data into aligned format.')
    parser.add_argument('remap_csv', type=argparse.FileType('r'),
                        help='<input> SAM output of bowtie2 in CSV format')
    parser.add_argument('aligned_csv', type=argparse.FileType('w'),
                        help='<output> CSV containing cleaned and merged reads')
    parser.add_argument('insert_csv', nargs='?', default=None, type=argparse.FileType('w'),
                        help='<output> CSV containing insertions relative to sample consensus')
    parser.add_argument('failed_csv', nargs='?', default=None, type=argparse.FileType('w'),
                        help='<output> CSV containing reads that failed to merge')
    parser.add_argument('-p', type=int, default=None, help='(optional) number of threads')
    parser.add_argument('--qcut', type=int, action='append', default=None, metavar='Q',
                        help='quality cutoff of the merge; repeat it for several '
                             '(default: {})'.format(' '.join(map(str, SAM2ALN_Q_CUTOFFS))))
    parser.add_argument('--clipping_csv', type=argparse.FileType('w'), default=None, metavar='FILE',
                        help='<output> CSV of soft-clipped positions that no mate aligns, '
                             'counted per consensus position')
    parser.add_argument('--conseq_ins_csv', type=argparse.FileType('w'), default=None, metavar='FILE',
                        help='<output> CSV of the insertions left out of the consensus, merged per '
                             'pair and counted per consensus position and string')
    parser.add_argument('--concordance_csv', type=argparse.FileType('w'), default=None, metavar='FILE',
                        help='<output> CSV of the positions both mates of a pair align: the pairs '
                             'and how many disagree there (mismatch, indel, nocall, unresolved)')
    parser.add_argument('--cycle_concordance_csv', type=argparse.FileType('w'), default=None,
                        metavar='FILE',
                        help='<output> CSV of the bases compared with the mate and found different, '
                             'per read and sequencing cycle and per read and quality')
    parser.add_argument('--strand_csv', type=argparse.FileType('w'), default=None, metavar='FILE',
                        help='<output> CSV of the strand support of every merged base: per position '
                             'and base the pairs with a supporting mate forward, reversed and both')
    return parser.parse_args()


def main():
    args = parseArgs()
    sam2aln(remap_csv=args.remap_csv, aligned_csv=args.aligned_csv, insert_csv=args.insert_csv,
            failed_csv=args.failed_csv, nthreads=args.p, q_cutoffs=args.qcut,
            clipping_csv=args.clipping_csv, conseq_ins_csv=args.conseq_ins_csv,
            concordance_csv=args.concordance_csv, cycle_concordance_csv=args.cycle_concordance_csv,
            strand_csv=args.strand_csv)


if __name__ == '__main__':
    main()
