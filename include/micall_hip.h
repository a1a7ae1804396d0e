/*
 * micall_hip.h -- C-ABI of libmicall_hip.so, the MI355X (gfx950) drop-in for
 * MiCall-Lite's iterative remap hot path.
 *
 * The reference crosses two boundaries on this path; every entry point below
 * replaces one of them (file:line into the reference):
 *
 *   1. the bowtie2 / bowtie2-build process boundary, reached through
 *      micall/utils/externals.py:106-125 (CommandWrapper.yield_output) and
 *      :185-203 (Bowtie2Build.build):
 *        bowtie2-build-s ... -f <fasta> <template>   prelim_map.py:106,
 *                                                    remap.py:695
 *          -> mh_index_build
 *        bowtie2 ... -1 R1 -2 R2 | -U R [--local]    prelim_map.py:134,
 *                                                    remap.py:734
 *          -> mh_reads_load / mh_reads_load_fastq (FASTQ ingest, once),
 *             mh_map (one mapping pass), mh_alns_fetch / mh_format_rows
 *             (the SAM lines bowtie2 would print), mh_map_counts (the
 *             per-line tallies remap.py:743-755 and :485-515 make);
 *   2. the pileup the reference runs in Python on the SAM text,
 *      remap.py:141-306 (sam_to_conseqs -> merge_reads -> apply_cigar /
 *      merge_pairs / merge_inserts -> update_counts)
 *          -> mh_rows_load (SAM rows read back from prelim.csv),
 *             mh_pileup, mh_pileup_fetch / mh_pileup_events,
 *             mh_pileup_export / mh_pileup_import (RCCL all-reduce between
 *             ranks, done by the caller on device buffers);
 *   3. the _gotoh2 C-extension boundary, micall/alignment/src/_gotoh2.c:544-607
 *      (align_wrapper, "ssiiisO")
 *          -> mh_gotoh_align;
 *   4. (next stage) sam2aln's Python merge of remap.csv,
 *      micall/core/sam2aln.py:395-478
 *          -> mh_sam2aln_csv / mh_sam2aln_csv_q (the list of q-cutoffs,
 *             :391-402), mh_sam2aln_output; mh_sam2aln_resident when the
 *             rows are the records of the mapping pass still on the device;
 *   5. (the stage before) censor_fastq.censor's per-base
 *      Python loop, micall/core/censor_fastq.py:32-102
 *          -> mh_censor_fastq / mh_censor_staged, mh_censor_output /
 *             mh_censor_write;
 *   6. (the stage after sam2aln) aln2counts' per-read loops,
 *      SequenceReport._count_reads (micall/core/aln2counts.py:115-172) and
 *      InsertionWriter.write (:748-811)
 *          -> mh_a2c_load_csv / mh_a2c_load_rows, mh_a2c_counts,
 *             mh_a2c_inserts; the nucleotide variants of the coordinate
 *             regions (:346-375, :537-549) -> mh_a2c_variants; the codons
 *             count_aminos drops (:595-603) -> mh_a2c_codon_detail; the
 *             amino acids one read links at chosen positions (no
 *             counterpart in the reference) -> mh_a2c_link; which minority
 *             variants single reads carry together, every pair of up to 256
 *             at once (no counterpart either) -> mh_a2c_gram.
 *
 * Conventions: every function returns 0 on success, -1 on traceback failure
 * (mh_gotoh_align only), -2 on out-of-memory, -3 on a bad argument, -4 on a
 * HIP runtime error, -5 when the HIP device or kernels are unavailable.
 * mh_last_error() describes the last failure of the calling thread.  No C++
 * exception and no exit() crosses this boundary.  All host buffers are owned
 * by the caller; device buffers are owned by the context.  One context per
 * device; calls on one context are not thread-safe, calls on different
 * contexts are independent (ctypes releases the GIL around each call).
 */
#ifndef MICALL_HIP_H
#define MICALL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_MAXOPS 128

enum { MH_E2E = 0, MH_LOCAL = 1 };          /* bowtie2 default / --local */
enum { MH_OP_M = 0, MH_OP_I = 1, MH_OP_D = 2, MH_OP_S = 4 };

/* Scoring knobs MiCall passes to bowtie2 (prelim_map.py:27-30,114-131). */
typedef struct {
    int mode;                 /* MH_E2E (prelim_map) or MH_LOCAL (remap) */
    int rdg_open, rdg_ext;    /* --rdg 10,3 */
    int rfg_open, rfg_ext;    /* --rfg 10,3 */
    int maxins;               /* -X 1200 */
} mh_params;

/* One SAM record of one read, fields as bowtie2 prints them.  Layout is
 * identical to oracle/og_mapper.h og_aln. */
typedef struct {
    int32_t ref, pos, rev, score, secbest, flag, mapq, rnext, pnext, tlen;
    int32_t sam_ref, sam_pos, xm, xo, xg, nm, ys, yt, yf, n_cigar;
    uint32_t cigar[MH_MAXOPS];   /* (len << 4) | op */
} mh_aln;

typedef struct mh_ctx mh_ctx;

int mh_version(void);
int mh_last_error(char *buf, size_t cap);
int mh_device_count(int *n);

int mh_ctx_create(int device, mh_ctx **out);
int mh_ctx_destroy(mh_ctx *ctx);
int mh_ctx_sync(mh_ctx *ctx);
/* the hipStream_t the context launches on (as an opaque handle) */
int mh_ctx_stream(mh_ctx *ctx, void **stream);

/* ---- reference set: replaces bowtie2-build ---------------------------- */
int mh_index_build(mh_ctx *ctx, int n_refs, const char *const *seqs, int seedlen);

/* ---- reads: replaces bowtie2's FASTQ input (-1/-2/-U) ------------------ */
/* Reads back to back; paired: reads 2p and 2p+1 are mates 1 and 2.  Kept
 * resident on the device (2-bit bases + N mask + qualities) across passes. */
int mh_reads_load(mh_ctx *ctx, int64_t n_reads, int paired, const uint8_t *seq,
                  const uint8_t *qual, const int64_t *offsets, const int32_t *lens);
/* Parse (gzip or plain) FASTQ files and load them; path2 may be NULL.
 * Keeps the read names (bowtie2 QNAME rules) for mh_format_rows. */
int mh_reads_load_fastq(mh_ctx *ctx, const char *path1, const char *path2, int64_t *n_reads);
/* One rank's block of a sharded run: the same parse (raw line count of the
 * whole file included), but only units (pairs, or reads when unpaired)
 * [U*part/parts, U*(part+1)/parts) of the U in the files stay resident;
 * *first_unit receives the block's first unit.  parts = 1 is
 * mh_reads_load_fastq. */
int mh_reads_load_fastq_part(mh_ctx *ctx, const char *path1, const char *path2, int part, int parts,
                             int64_t *n_reads, int64_t *first_unit);
int mh_reads_count(mh_ctx *ctx, int64_t *n_reads, int *paired);

/* ---- sharded FASTQ ingest (host only; replaces each rank's decode of the
 * whole file: the reference streams the FASTQ once per pass,
 * prelim_map.py:114-134 / censor_fastq.py:58-96) ---------------------------
 * mh_fastq_open_part decodes part `part` of `parts` of a FASTQ file (path,
 * or an open descriptor when path is NULL): with parts > 1 the gzip members
 * starting in the part's byte range (mode 1), the byte range of a plain file
 * (mode 2); the whole file otherwise (mode 0; also with parts == 1).
 * info[10]: mode, first and end file offset read, decoded bytes, newlines in
 * them, ends with '\n', starts with '\n', file bytes decoded, file size,
 * wall time (microseconds). */
typedef struct mh_fastq mh_fastq;
int mh_fastq_open_part(const char *path, int fd, int part, int parts, mh_fastq **out, int64_t *info);
/* The ranks' test for a single gzip member: info[3] = is gzip, file size,
 * 1 if a gzip member starts inside part `part`'s byte range (past offset
 * 0).  Scans 1/parts of the file; no decode. */
int mh_fastq_scan_part(const char *path, int fd, int part, int parts, int64_t *info);
/* Part `part` of `parts` of a FASTQ file that is one gzip member (bcl2fastq's
 * layout), decoded without any other part's bytes (the reference reads the
 * file once per pass, prelim_map.py:114-134; censor_fastq.py:58-96):
 *   open    info[7]: this part's first deflate block start (bit; -1 if its
 *           share of the compressed bytes holds none: not splittable), the
 *           stream's end bit, the trailer's CRC-32 and size, spans, file
 *           size, microseconds;
 *   decode  up to end_bit (the next part's first block start, or the
 *           stream's end bit for the last part); info[2]: text bytes (-1:
 *           not decodable this way), microseconds;
 *   tail    with `window` = the previous part's last 32768 text bytes (NULL
 *           for part 0), this part's last 32768 text bytes into tail[32768]
 *           (the next part's window);
 *   finish  the rest of the text resolved; info[11]: the mh_fastq_open_part
 *           fields with mode 3 and file offsets c0 / c1 as given, then the
 *           CRC-32 of this part's text (the caller checks the combined CRC
 *           and size against the trailer).
 * Each returns 0, -1 (not resolvable: fall back), -2 out of memory, -3 bad
 * arguments. */
int mh_fastq_member_open(const char *path, int fd, int part, int parts, mh_fastq **out, int64_t *info);
int mh_fastq_member_decode(mh_fastq *fq, int64_t end_bit, int64_t *info);
int mh_fastq_member_tail(mh_fastq *fq, const char *window, char *tail);
int mh_fastq_member_finish(mh_fastq *fq, const char *window, int64_t c0, int64_t c1, int64_t *info);
/* Record starts of the held text, a record being four lines: line0 = lines
 * of the file before its first byte, starts_line = 1 if that byte starts a
 * line.  out[5]: offset of the first record start (the size if none),
 * record starts, that start's line number in the file (-1 if none), 1 if a
 * blank line sits where a record starts (the ingest's parser would skip it),
 * 1 if the text ends in an unterminated record-start line that is only a
 * '\r'. */
int mh_fastq_frame(mh_fastq *fq, int64_t line0, int starts_line, int64_t *out5);
/* byte offset of framed record k (k = the record count: the text's size) */
int mh_fastq_record_offset(mh_fastq *fq, int64_t k, int64_t *off);
/* the held text becomes front + text[lo, hi) + back (framing is dropped) */
int mh_fastq_splice(mh_fastq *fq, int64_t lo, int64_t hi, const char *front, int64_t flen,
                    const char *back, int64_t blen);
/* the held text (valid until the handle changes or is closed) */
int mh_fastq_view(mh_fastq *fq, const char **data, int64_t *len);
int mh_fastq_close(mh_fastq *fq);
/* Host-only parse of staged FASTQ text (fq2 NULL: unpaired) as the loader
 * parses it (records, bowtie2 QNAMEs, SEQ / QUAL; the texts are kept): the
 * QNAMEs '\n'-terminated in names, the bases and qualities concatenated,
 * the lengths per read (mates interleaved).  With names, seq, qual or lens
 * NULL only the sizes are returned.  For tests of the ingest without a
 * device. */
int mh_fastq_parse(mh_fastq *fq1, mh_fastq *fq2, char *names, size_t names_cap, uint8_t *seq,
                   uint8_t *qual, size_t bases_cap, int32_t *lens, int64_t reads_cap, int64_t *n_reads,
                   int64_t *n_bases, size_t *names_used);
/* Load the reads of staged FASTQ text: units [range[0], range[1]) of fq1's
 * records and [range[2], range[3]) of fq2's (-1, -1: all of them; the two
 * counts must agree), mates interleaved when fq2 is given.  The records are
 * parsed as mh_reads_load_fastq parses a file; the texts are moved into the
 * context (the handles are left empty).  fastq_lines1 is the newline count
 * of the whole FASTQ 1 (mh_reads_fastq_lines, raw_count). */
int mh_reads_load_staged(mh_ctx *ctx, mh_fastq *fq1, mh_fastq *fq2, const int64_t *range4,
                         int64_t fastq_lines1, int64_t *n_reads);
/* newlines in FASTQ 1 of the last mh_reads_load_fastq (the `gunzip -c | wc
 * -l` of LineCounter, externals.py:206-231; raw_count = lines / 2). */
int mh_reads_fastq_lines(mh_ctx *ctx, int64_t *lines1);

/* ---- one mapping pass: replaces `bowtie2 [--local] ...` ---------------- */
int mh_map(mh_ctx *ctx, const mh_params *par);
int mh_alns_fetch(mh_ctx *ctx, int64_t first, int64_t n, mh_aln *out);
/* Per-reference tallies of the last pass (n_refs entries each):
 *   lines[r]     SAM lines with RNAME r           (prelim count, remap.py:494)
 *   filtered[r]  mapped lines with a >50-base M run (remap.py:500-506)
 *   mapped[r]    mapped lines with RNAME r        (new_counts, remap.py:755)
 *   first_row[r] first line index with RNAME r, -1 if none
 *   first_mapped[r] first mapped line with RNAME r (Counter order), -1 if none
 * and *unmapped = unmapped lines (remap.py:743-753); star_lines / star_first =
 * number of / first line with RNAME '*'. */
int mh_map_counts(mh_ctx *ctx, int64_t *lines, int64_t *filtered, int64_t *mapped,
                  int64_t *first_row, int64_t *first_mapped, int64_t *unmapped,
                  int64_t *star_lines, int64_t *star_first);
/* Work done by the last mh_map: out[0] reads, out[1] banded extensions
 * (candidates aligned by the DP, up to 31 diagonals x read length cells each,
 * mate rescues included), out[2] CIGAR pool words reserved (per-wave
 * chunks), out[3] extensions resolved by the ungapped fast path (no DP),
 * out[4] mate-rescue candidates found.  A rescue candidate on a (strand,
 * reference, diagonal) the main pass already extended for that mate, and
 * failed on, is not extended again: it counts in out[4] but not in out[1]. */
int mh_map_stats(mh_ctx *ctx, int64_t *out5);
/* Test entry point: *out = the mate-rescue candidates of the last mh_map that
 * were not extended again (see mh_map_stats; out[4] - *out ran through the
 * DP).  The caller's five-value buffer of mh_map_stats cannot grow, hence
 * the separate call. */
int mh_test_rescue_skipped(mh_ctx *ctx, int64_t *out);
/* Test entry point (not a tuning knob): start the grow-and-retry buffers of
 * every later call at these capacities (0 = the library's own sizing):
 * the CIGAR pool of mh_map (uint32 words), the pileup's insertion-token
 * events and their bytes (mh_pileup), the distinct-token bytes of the token
 * aggregation (mh_pileup_events, mh_pileup_fetch).  A pass that needs more
 * takes the retry path, which the parity tests then check bit for bit.  The
 * call drops the buffers (and the last pass's records) so the next call
 * sizes them again. */
int mh_test_set_capacities(mh_ctx *ctx, int64_t cigar_pool_words, int64_t pileup_events,
                           int64_t pileup_event_bytes, int64_t token_bytes);
/* Test entry point, read-only: the launch shapes of the last mh_pileup and of
 * the token aggregation behind it (mh_pileup_dims / mh_pileup_events), so a
 * test can assert that its input took the path it was built for.
 *   out16[0..6]  constants: reference span per mate expanded with all loads
 *                in flight (PU_XCH * 64), MH_MAXOPS, PU_INSBUF (merged
 *                insertion bytes per unit), PU_MAXINS, TOK_LDS_SLOTS,
 *                TOK_LDS_KEYS, MH_PILEUP_SLACK
 *   out16[7..10] k_pileup: blocks, waves per block, LDS window words, units
 *   out16[11..14] k_tok_insert blocks, k_tok_count blocks, events, distinct keys
 *                (0 until the tokens were aggregated)
 *   out16[15]    references of that pileup
 *   win_len[r]   r < n_refs: positions of reference r's LDS window, 0 without
 *                one, -1 for a reference mh_pileup_only left out
 * ctx may be NULL: the constants alone. */
int mh_test_pileup_info(mh_ctx *ctx, int64_t *out16, int n_refs, int32_t *win_len);
/* Test entry point, read-only: the constants that size k_s2a_merge's launch
 * and the shape of the last one (mh_sam2aln_csv and the other sam2aln calls),
 * so a test can size its input by them and assert the path it took.
 *   out16[0..6]  constants: LDS bytes of one block at most (160 KiB), blocks
 *                of one launch at most (256 * 64), waves per block while they
 *                fit (4), slots of the grouping table at least (1024),
 *                q-cutoffs of one call at most, and the bytes a wave keeps in
 *                LDS per reference position (4) and per CIGAR op (16):
 *                wave_bytes = 4 * span_cap + 16 * (ops_cap + 1), rounded up
 *                to 16, span_cap = the longest reference span rounded up to 16
 *   out16[7..14] the last launch: span_cap, ops_cap, wave_bytes, waves per
 *                block, blocks, merge units, q-cutoffs, grouping table slots
 *                (waves per block, blocks and slots 0 for a call refused
 *                before the launch; all 0 before the first call)
 *   out16[15]    key_bits as mh_test_set_sam2aln left it
 * ctx may be NULL: the constants alone. */
int mh_test_sam2aln_info(mh_ctx *ctx, int64_t *out16);
/* Test entry point (not a tuning knob), for the sam2aln calls that follow:
 * key_bits (8..64) = bits of the merged-sequence hash used as the grouping
 * key, 64 in the product; fewer make distinct sequences share a key, which
 * the call must report (-4, "hash collision"), never merge.  max_blocks caps
 * the blocks of k_s2a_merge (0: the library's own cap), so that one wave
 * merges many units in turn.  The insertion table of mh_sam2aln_conseq_ins
 * narrows its key the same way.  (64, 0) restores the product's values. */
int mh_test_set_sam2aln(mh_ctx *ctx, int key_bits, int64_t max_blocks);
/* Test entry point: on != 0 gives every reference set of later
 * mh_index_build calls the same cache signature, so only the comparison of
 * the cached bytes tells two sets apart. */
int mh_test_force_index_collision(mh_ctx *ctx, int on);
/* Retries taken so far by those paths: out4[0] CIGAR pool (a mapping pass
 * run again from k_seed), out4[1] pileup events, out4[2] token bytes,
 * out4[3] Gotoh batches run again after a strip's wait timed out. */
int mh_retry_counts(mh_ctx *ctx, int64_t *out4);
/* Test entry point: k_gotoh's first attempt of every later batch gives up a
 * neighbour wait after `ticks` of the 100 MHz real-time clock (0: the
 * default 20 s), so the timeout-and-retry path of mh_gotoh_align_batch runs. */
int mh_test_set_gotoh_wait(mh_ctx *ctx, int64_t ticks);
/* The 20 int32 header fields of mh_aln (no CIGAR) for reads [first, first+n). */
int mh_recs_fetch(mh_ctx *ctx, int64_t first, int64_t n, int32_t *out20);
/* Fields [field0, field0 + nfields) of records [first, first + n) (the
 * mh_recs_fetch field order), nfields int32 per record. */
int mh_recs_fetch_fields(mh_ctx *ctx, int64_t first, int64_t n, int field0, int nfields, int32_t *out);
/* SAM text for reads order[first .. first+n) (order NULL: reads first ..
 * first+n-1): style 0 = tab-separated SAM with
 * optional tags, style 1 = the 11 CSV columns prelim.csv / remap.csv hold
 * (csv.QUOTE_MINIMAL).  Needs names from mh_reads_load_fastq or
 * mh_reads_set_names.  *used = bytes written; -2 if cap is too small.
 * buf NULL: a size query; *used = the text's size, and the text is kept
 * for the next call with the same arguments (a copy into buf, no
 * reformatting).  Rows are formatted on host threads. */
int mh_reads_set_names(mh_ctx *ctx, int64_t n, const char *const *names);
int mh_format_rows(mh_ctx *ctx, int style, const int64_t *order, int64_t first, int64_t n,
                   const char *const *refnames, char *buf, size_t cap, size_t *used);
/* Rows order[0 .. n) (order NULL: reads 0 .. n - 1) formatted as style 0 /
 * 1 text (as mh_format_rows) in n_seg segments, segment s being rows
 * seg_rows[s] .. seg_rows[s + 1] (ascending, seg_rows[n_seg] <= n).  The
 * text is kept; seg_bytes[s] = its size per segment.  A sharded run
 * all-gathers the sizes to place every rank's segments in one file. */
int mh_format_segments(mh_ctx *ctx, int style, const int64_t *order, int64_t n,
                       const char *const *refnames, int n_seg, const int64_t *seg_rows,
                       int64_t *seg_bytes);
/* Write the text of the last mh_format_segments to fd, segment s at file
 * offset seg_off[s] (pwrite on host threads; the file position is not
 * used); crc[s] = crc32 of segment s (crc NULL: none).  Frees the text. */
int mh_write_segments(mh_ctx *ctx, int fd, const int64_t *seg_off, uint32_t *crc);
/* crc32 (zlib's) of A then B, from crc32(A), crc32(B) and B's length */
uint32_t mh_crc32_combine(uint32_t a, uint32_t b, int64_t len_b);
/* crc32 of a whole open file and its size (a read-back check) */
int mh_file_crc32(int fd, int64_t *size, uint32_t *crc);
/* Host wall time (ms) per phase of the file path since the last reset:
 * MH_PHASE_INFLATE (FASTQ gunzip), _PARSE (record scan, names, copies),
 * _UPLOAD (H2D + 2-bit packing), _FORMAT (SAM / CSV text), _WRITE (pwrite).
 * ms[MH_PHASES]; reset != 0 zeroes them after the copy. */
enum { MH_PHASE_INFLATE = 0, MH_PHASE_PARSE = 1, MH_PHASE_UPLOAD = 2, MH_PHASE_FORMAT = 3,
       MH_PHASE_WRITE = 4, MH_PHASES = 5 };
int mh_phase_times(mh_ctx *ctx, double *ms, int reset);
/* The same rows written straight to an open file descriptor at `offset`
 * (pwrite, no copy through the caller): *written bytes, *crc their crc32
 * (crc NULL: none).  The rows are formatted in chunks on host threads while
 * one thread writes the finished chunks in order.  The caller moves its
 * file position past them. */
int mh_write_rows_crc(mh_ctx *ctx, int style, const int64_t *order, int64_t first, int64_t n,
                      const char *const *refnames, int fd, int64_t offset, int64_t *written,
                      uint32_t *crc);

/* ---- pileup: replaces sam_to_conseqs' counting (remap.py:141-306) ------ */
/* External SAM rows (e.g. prelim.csv read back, remap.py:474-498).
 * units: n_units pairs of row indices as matchmaker (remap.py:853-889)
 * yields them, -1 for a missing mate.  seq/qual as printed in SAM. */
int mh_rows_load(mh_ctx *ctx, int64_t n_rows, const int32_t *flag, const int32_t *ref,
                 const int32_t *pos, const int32_t *cigar_off, const int32_t *n_cigar,
                 const uint32_t *cigar, const uint8_t *seq, const uint8_t *qual,
                 const int64_t *offsets, const int32_t *lens, int64_t n_units,
                 const int64_t *unit_rows);
/* prelim.csv text (prelim_map.py:142-151) read back as remap() does
 * (remap.py:474-498): csv quoting, rname -> index into refnames (the @SQ
 * set), matchmaker pairing by qname, upload as rows.  mh_rows_info then
 * gives per row: name id (>= 0 index into refnames, < 0 other names such
 * as '*'), flag, longest M run (is_short_read, remap.py:70-83), ref index. */
int mh_rows_load_csv(mh_ctx *ctx, const char *text, int64_t len, int n_refs,
                     const char *const *refnames, int64_t *n_rows, int64_t *n_units,
                     int32_t *n_present);
/* out4 per row: name id, flag, longest M run, compact ref id; present[k] =
 * @SQ index of compact ref k; unknown = '\n'-joined names outside @SQ. */
int mh_rows_info(mh_ctx *ctx, int32_t *out4, int32_t *present, char *unknown, size_t cap);
/* source 0 = alignments of the last mh_map (units = pairs / reads),
 * source 1 = rows from mh_rows_load.  n_refs/ref_lens size the dense
 * counters (positions 1..ref_lens[r] + MH_PILEUP_SLACK). */
#define MH_PILEUP_SLACK 2048
int mh_pileup(mh_ctx *ctx, int source, int q_cutoff, int n_refs, const int32_t *ref_lens);
/* mh_pileup counting only the references sel[0 .. n_sel) (n_sel < 0: all):
 * the units mapped to any other are skipped and its counters, read count
 * and positions stay empty.  The prelim pass builds only the seed-group
 * winners' consensuses (remap.py:531-541 keeps those of build_conseqs'
 * output), so their pileup alone is needed; every reference is counted
 * independently of the others, so theirs are the same. */
int mh_pileup_only(mh_ctx *ctx, int source, int q_cutoff, int n_refs, const int32_t *ref_lens, int n_sel,
                   const int32_t *sel);
/* Watched positions: the debug_reports of sam_to_conseqs (remap.py:169-225,
 * 302-306).  Sets the (reference index, 1-based position) keys of the next
 * mh_pileup calls, n_keys = 0 clears them; -3 above MH_WATCH_MAXKEYS keys or
 * for a position < 1.  A watched pileup also fills, per key, a histogram of
 * base (A C G T) x quality character (MH_WATCH_QBINS bins, ' ' .. '~') over
 * the merged pairs that counted a base there, the quality being qual1's or
 * qual2's as remap.py:305 picks it.  A key on a reference outside the
 * pileup's n_refs, or past its counters, never counts.  mh_pileup_only with
 * a selection refuses to run watched (-3). */
#define MH_WATCH_MAXKEYS 1024
#define MH_WATCH_QBINS 95
int mh_pileup_watch(mh_ctx *ctx, int n_keys, const int32_t *refs, const int32_t *poss);
/* The histogram of the last watched mh_pileup (remap.py:169-225, 302-306),
 * keys in the caller's order: counts[n_keys][4][MH_WATCH_QBINS] and, per
 * cell, the first matchmaker unit that added to it (INT64_MAX: none), which
 * gives the insertion order of the reference's Counter. */
int mh_pileup_watch_fetch(mh_ctx *ctx, uint32_t *counts, int64_t *first_unit);
/* SAM text read as remap.matchmaker(samfile, include_singles=True) reads it
 * (remap.py:853-889) and uploaded as rows, as mh_rows_load_csv does for
 * prelim.csv: '@' lines are headers, every SN of an @SQ line (fields split
 * at the first ':') names a reference; only '\n' is stripped; the first
 * eleven tab fields are used; a row whose RNAME is no @SQ name is dropped;
 * rows pair by QNAME, pairs in the order of their second rows, then the
 * singles.  mh_sam_info gives the names and, per reference, the largest
 * reference end (POS - 1 + M + D) of a mapped row. */
int mh_rows_load_sam(mh_ctx *ctx, const char *text, int64_t len, int64_t *n_rows,
                     int64_t *n_units, int32_t *n_refs, size_t *names_bytes);
/* after mh_rows_load_sam: names '\n'-joined (names_bytes + 1 bytes), ends[n_refs] */
int mh_sam_info(mh_ctx *ctx, char *names, size_t cap, int32_t *ends);
/* Host-only parse of SAM text as mh_rows_load_sam parses it, no device: the
 * sizes first (any array NULL), then the caller's arrays.  Per kept row:
 * flag, reference index, POS, CIGAR ops ((len << 4) | op; an unmapped row
 * has none, an invalid or over-long CIGAR is the single op 3) at cigar_off,
 * SEQ / QUAL bytes (QUAL cut or padded with 'J' to SEQ's length) at
 * seq_off; units as mh_rows_load takes them; names '\n'-joined.  Returns
 * -3 (with a message) for a line with fewer than eleven fields or a FLAG /
 * POS that is no integer, where the reference raises. */
typedef struct {
    int64_t n_rows, n_units, n_cigar, n_bases;
    int32_t n_refs;
    size_t names_bytes;
} mh_sam_sizes;
int mh_sam_parse(const char *text, int64_t len, mh_sam_sizes *sizes, int32_t *flag, int32_t *ref,
                 int32_t *pos, int32_t *cigar_off, int32_t *n_cigar, uint32_t *cigar,
                 int64_t *seq_off, int32_t *seq_len, uint8_t *seq, uint8_t *qual, int64_t *units,
                 char *names, int32_t *ends);
/* Host-only parse of prelim.csv text as mh_rows_load_csv parses it, no
 * device: the sizes first (any array NULL), then the caller's arrays.  Per
 * data row, in file order: the arrays mh_rows_load takes (ref is the compact
 * reference id; CIGAR ops and QUAL as mh_sam_parse gives them), units, and
 * what mh_rows_info gives: info[n_rows][4], present[n_present], unknown
 * '\n'-joined (unknown_bytes + 1 bytes).  threads: host threads the text is
 * cut over, 0 for the default; the result does not depend on it.  Returns -3
 * (with a message) for an empty text, a missing column or a short row. */
typedef struct {
    int64_t n_rows, n_units, n_cigar, n_bases;
    int32_t n_present;
    size_t unknown_bytes;
} mh_prelim_sizes;
int mh_prelim_parse(const char *text, int64_t len, int n_refs, const char *const *refnames,
                    int threads, mh_prelim_sizes *sizes, int32_t *flag, int32_t *ref, int32_t *pos,
                    int32_t *cigar_off, int32_t *n_cigar, uint32_t *cigar, int64_t *seq_off,
                    int32_t *seq_len, uint8_t *seq, uint8_t *qual, int64_t *units, int32_t *info,
                    int32_t *present, char *unknown);
/* dense: n_refs x cap x 4 int32 counts of A,C,G,T at positions 1..cap;
 * nflag/dflag: n_refs x cap bytes ('N' seen -> count -1, '-' seen -> -2);
 * read_counts: merged pairs per ref; first_unit: first merged unit index
 * per ref (-1 if none); max_pos: largest position touched per ref. */
int mh_pileup_dims(mh_ctx *ctx, int *n_refs, int32_t *cap, int64_t *n_events,
                   int64_t *event_bytes);
int mh_pileup_fetch(mh_ctx *ctx, int32_t *dense, uint8_t *nflag, uint8_t *dflag,
                    int64_t *read_counts, int64_t *first_unit, int32_t *max_pos);
/* The counter rows of n_sel references in one call (one stream
 * synchronisation): dense / nflag / dflag are the whole (n_refs x cap [x 4])
 * arrays, and reference refs[k]'s rows 0 .. max_pos - 1 are written (its
 * positions 1 .. max_pos; past its last counted position every row is zero,
 * and those rows are left as the caller zeroed them). */
int mh_pileup_fetch_refs(mh_ctx *ctx, int n_sel, const int32_t *refs, int32_t *dense, uint8_t *nflag,
                         uint8_t *dflag);
/* Sparse tokens (base + insertion with len % 3 == 0), aggregated over the
 * pileup: n_events (mh_pileup_dims) distinct (ref, pos, token) entries in
 * (ref, pos, token) order, each with the number of merged pairs that voted
 * for it; the token is pool[tok_off[e] .. tok_off[e] + tok_len[e]). */
int mh_pileup_events(mh_ctx *ctx, int32_t *ref, int32_t *pos, int32_t *tok_off,
                     int32_t *tok_len, int64_t *count, char *pool);
/* Multi-GPU: the caller all-reduces three device buffers with RCCL after
 * mh_pileup_export and hands them to mh_pileup_import.  Only the rows of the
 * n_sel references in sel (the same list on every rank: those with data on
 * any rank) travel:
 *   sum   int32, SUM: dense rows of sel, then read_counts of every ref
 *   max   int32, MAX: max_pos of every ref, then -(first_unit + unit_base)
 *         (unit_base = this rank's first unit index: the MAX yields the
 *         global first unit, i.e. the reference's refmap order)
 *   flags uint8, MAX: nflag rows, then dflag rows of sel (0/1: MAX = OR)
 * mh_pileup_exchange_bytes gives the three sizes. */
int mh_pileup_exchange_bytes(mh_ctx *ctx, int n_sel, int64_t *sum_bytes, int64_t *max_bytes,
                             int64_t *flag_bytes);
int mh_pileup_export(mh_ctx *ctx, int n_sel, const int32_t *sel, int64_t unit_base,
                     void *dev_sum, void *dev_max, void *dev_flags);
int mh_pileup_import(mh_ctx *ctx, int n_sel, const int32_t *sel, const void *dev_sum,
                     const void *dev_max, const void *dev_flags);
/* Insertion-token events across ranks (the sparse side table of the pileup):
 * mh_pileup_event_bytes gives this rank's raw event count and pool bytes;
 * mh_pileup_events_export copies them (4 int32 per event, then the bytes)
 * into caller device buffers; after an all-gather of those buffers,
 * mh_pileup_events_import replaces the rank's events by the concatenation of
 * `parts` parts (part p at dev_events + p * events_stride int32 words and
 * dev_pool + p * pool_stride bytes), so mh_pileup_events aggregates every
 * rank's tokens. */
int mh_pileup_event_bytes(mh_ctx *ctx, int64_t *n_events, int64_t *pool_bytes);
int mh_pileup_events_export(mh_ctx *ctx, void *dev_events, void *dev_pool);
int mh_pileup_events_import(mh_ctx *ctx, int parts, const int64_t *n_events,
                            const int64_t *pool_bytes, const void *dev_events,
                            int64_t events_stride, const void *dev_pool, int64_t pool_stride);

/* ---- sam2aln: replaces sam2aln.sam2aln (sam2aln.py:395-478) ----------- */
/* remap.csv text (the SAM columns remap() writes) read as DictReader does,
 * paired by qname (matchmaker, sam2aln.py:291-312), every pair merged on the
 * device (parse_sam, :315-391: apply_cigar, merge_pairs at q_cutoff, the
 * prop_N > max_prop_n test) and identical merged sequences counted per rname
 * (:449-456).  MiCall passes q_cutoff 15 and max_prop_n 0.5
 * (SAM2ALN_Q_CUTOFFS, MAX_PROP_N).  Fails (-3, message as the reference's
 * RuntimeError) on a CIGAR apply_cigar rejects.  *n_units = matchmaker pairs. */
int mh_sam2aln_csv(mh_ctx *ctx, const char *text, int64_t len, int q_cutoff, double max_prop_n,
                   int64_t *n_units);
/* mh_sam2aln_csv with SAM2ALN_Q_CUTOFFS as a list (sam2aln.py:25): one
 * device pass merges every pair at each of the n_cut cutoffs (parse_sam's
 * `for qcut in SAM2ALN_Q_CUTOFFS`, :391-402; apply_cigar and the insert rows
 * once per pair).  aligned.csv then holds one group per (rname, qcut), a
 * rname's groups in the order in which each cutoff first received a passing
 * sequence (:446-452), and failed.csv one manyNs row for a pair that failed
 * at any cutoff (:381-389).  -3, with a message, for n_cut outside 1..8, a
 * cutoff outside 0..93 or a repeated cutoff. */
int mh_sam2aln_csv_q(mh_ctx *ctx, const char *text, int64_t len, int n_cut, const int32_t *q_cutoffs,
                     double max_prop_n, int64_t *n_units);
/* CSV text of the last mh_sam2aln_csv / mh_sam2aln_csv_q: which 0 = aligned.csv, 1 =
 * insert.csv, 2 = failed.csv (DictWriter, '\n' line ends, with header).
 * buf NULL: only *used = bytes needed. */
int mh_sam2aln_output(mh_ctx *ctx, int which, char *buf, size_t cap, size_t *used);
/* mh_sam2aln_csv on the whole of a regular file (fd, mmap'd from offset 0):
 * 0, or 1 when the file holds '\r' (a text-mode read would translate it;
 * the caller reads the file itself), or an error. */
int mh_sam2aln_file(mh_ctx *ctx, int fd, int q_cutoff, double max_prop_n, int64_t *n_units);
/* mh_sam2aln_csv_q on the whole of a regular file, as mh_sam2aln_file. */
int mh_sam2aln_file_q(mh_ctx *ctx, int fd, int n_cut, const int32_t *q_cutoffs, double max_prop_n,
                      int64_t *n_units);
/* sam2aln over the records of the last mh_map and the resident reads (what
 * remap() wrote as remap.csv, one row per read in read order), merged at
 * n_cut cutoffs as mh_sam2aln_csv_q; refnames = the @SQ names of that pass.
 * The rows are built on the device (k_s2a_stage) instead of parsed and
 * uploaded; the outputs are those of mh_sam2aln_csv_q on that file.
 * -3 with a message when no mapping pass or no read names are resident.
 * 1 (nothing computed) when such a file's rows would pair otherwise than
 * the reads do -- mates with two QNAMEs, or unpaired reads whose QNAMEs may
 * repeat: the caller parses the file. */
int mh_sam2aln_resident(mh_ctx *ctx, int n_refs, const char *const *refnames, int n_cut,
                        const int32_t *q_cutoffs, double max_prop_n, int64_t *n_units);
/* Test entry point: SEQ / QUAL of rows [first, first + n) as the last
 * mh_sam2aln_resident staged them, back to back, with their lengths.
 * *used = the bytes of either; seq NULL only sizes. */
int mh_sam2aln_resident_rows(mh_ctx *ctx, int64_t first, int64_t n, int32_t *len,
                             uint8_t *seq, uint8_t *qual, size_t cap, size_t *used);
/* Output `which` (as mh_sam2aln_output) written to fd at offset with
 * pwrite (the descriptor's own offset is not used); *written = its size.
 * Not sized before (no mh_sam2aln_output size query), it is formatted and
 * written in one pass, the writes overlapping the formatting. */
int mh_sam2aln_write(mh_ctx *ctx, int which, int fd, int64_t offset, int64_t *written);
/* clipping.csv of the last sam2aln call on this context (mh_sam2aln_csv_q,
 * mh_sam2aln_file_q, mh_sam2aln_resident or mh_sam2aln_part): per reference
 * and 1-based position the number of merged units that soft-clip the
 * position while no mate aligns it (refname,pos,count; names sorted as
 * strings, then positions; '\n' line ends; positions may be <= 0 or past
 * the reference's end).  A unit counts when it reaches the merge (its cause
 * is none of unmatched, badCigar, 2refs), once whatever the q-cutoffs.
 * Nothing is computed before the first of these three calls asks: the pass
 * (k_s2a_clip, k_s2a_clip_scan) then runs over the rows and units the call
 * left on the device, so ask before the next sam2aln or mapping call.
 * buf NULL: only *used = bytes needed.  -3 with a message when a
 * reference's rows span more than 2^26 positions. */
int mh_sam2aln_clipping(mh_ctx *ctx, char *buf, size_t cap, size_t *used);
/* The same text written to fd at offset with pwrite; *written = its size. */
int mh_sam2aln_clipping_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written);
/* The same counts as arrays in the text's row order: name_id indexes the
 * call's reference names in first-seen order over its units (the order
 * mh_sam2aln_part_names prints).  *n = rows; arrays NULL: only *n. */
int mh_sam2aln_clip_counts(mh_ctx *ctx, int32_t *name_id, int64_t *pos, int32_t *count, int64_t cap,
                           int64_t *n);
/* Mate concordance of the last sam2aln call on this context, over the paired
 * units that reach the merge (the units clipping.csv counts, FLAG bit 1 set),
 * whatever the q-cutoffs.  Each mate is expanded as apply_cigar expands it.
 * which 0, concordance.csv (refname,pos,overlap,mismatch,indel,nocall,
 * unresolved): per reference and 1-based position both mates align (M or D),
 * the units (overlap), those whose two bytes differ -- nocall when either is
 * 'N', else indel when either is '-', else mismatch -- and those that differ
 * with qualities closer than 5 (unresolved); rows with overlap > 0, names
 * sorted as strings, then positions.  which 1, cycle_concordance.csv
 * (read,by,value,compared,mismatch): per read (1: FLAG 0x40, else 2) and
 * sequencing cycle (by = cycle) or quality - 33 (by = quality) the bases
 * compared with the mate's base -- both read bases, neither 'N' -- and found
 * different; rows with compared > 0, by read, cycles before qualities, then
 * value.  '\n' line ends.  Nothing is computed before the first of these three
 * calls asks: the pass (k_s2a_conc, k_s2a_conc_scan) then runs once over the
 * rows and units the call left on the device, so ask before the next sam2aln
 * or mapping call.  buf NULL: only *used = bytes needed.  -3 with a message
 * naming the reference when its paired rows span more than 2^26 positions. */
int mh_sam2aln_concordance(mh_ctx *ctx, int which, char *buf, size_t cap, size_t *used);
/* The same text written to fd at offset with pwrite; *written = its size. */
int mh_sam2aln_concordance_write(mh_ctx *ctx, int which, int fd, int64_t offset, int64_t *written);
/* The same counts as arrays in the texts' row order.  Positions: name_id (as
 * in mh_sam2aln_clip_counts), pos and five counts per row (overlap, mismatch,
 * indel, nocall, unresolved); *n = rows.  Reads: five int64 per row (read, by
 * with 0 cycle and 1 quality, value, compared, mismatch); *read_n = rows.
 * Arrays NULL: only *n and *read_n. */
int mh_sam2aln_conc_counts(mh_ctx *ctx, int32_t *name_id, int64_t *pos, int32_t *counts5, int64_t cap,
                           int64_t *n, int64_t *reads5, int64_t read_cap, int64_t *read_n);
/* Strand support of the last sam2aln call on this context: strand.csv
 * (refname,qcut,pos,A_fwd,A_rev,A_both,C_fwd,...,del_fwd,del_rev,del_both).
 * A unit counts at the q-cutoffs at which it gives aligned.csv a sequence.
 * At index j of its merged string (position j + 1) with merged character m in
 * "ACGT-", a mate supports m when its own expansion (apply_cigar at POS)
 * holds the byte m there, whatever its quality; the unit adds 1 to m_fwd when
 * a supporting mate has FLAG 0x10 clear, 1 to m_rev when one has it set, 1 to
 * m_both when both hold.  So m_fwd + m_rev - m_both is the count of the
 * aligned.csv rows that hold m there.  Rows with any count, names sorted as
 * strings, then the call's cutoffs in its order, then positions; '\n' line
 * ends.  Nothing is computed before the first of these three calls asks: the
 * pass (k_s2a_strand, k_s2a_strand_scan) then runs once over the rows, units
 * and merge results the call left on the device, so ask before the next
 * sam2aln or mapping call.  buf NULL: only *used = bytes needed.  -3 with a
 * message naming the reference when its rows span more than 2^26 positions,
 * and when the counters of all references and cutoffs would exceed 2^30
 * bytes; the call's other outputs stay available. */
int mh_sam2aln_strand(mh_ctx *ctx, char *buf, size_t cap, size_t *used);
/* The same text written to fd at offset with pwrite; *written = its size. */
int mh_sam2aln_strand_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written);
/* The same counts as arrays in the text's row order: name_id (as in
 * mh_sam2aln_clip_counts), the cutoff, pos and fifteen counts per row in the
 * columns' order; *n = rows.  Arrays NULL: only *n. */
int mh_sam2aln_strand_counts(mh_ctx *ctx, int32_t *name_id, int32_t *qcut, int64_t *pos,
                             int32_t *counts15, int64_t cap, int64_t *n);
/* conseq_ins.csv of the last sam2aln call on this context: the insertions
 * that remap's last pass left out of the consensus, merged per unit as the
 * reference's merge_inserts merges them and counted per distinct string
 * (refname,qcut,pos,insert,count; names sorted as strings, then the cutoff,
 * then pos, then count descending, then the string as bytes; '\n' line
 * ends).  pos is the 0-based consensus coordinate of the base that follows
 * the insertion (the 1-based position it follows; 0: before the first
 * base), not insert.csv's read-derived pos.  A unit counts at the cutoffs at
 * which it contributes a sequence to aligned.csv.  Nothing is computed
 * before the first of these three calls asks: the pass (k_s2a_ins_rec,
 * k_s2a_ins_merge, k_s2a_ins_tab and the merge's grouping kernels) then runs
 * over the rows, units and merge results the call left on the device, so
 * ask before the next sam2aln or mapping call.  buf NULL: only *used = bytes
 * needed.  -3 with a message naming the read when an inserted byte is '-'. */
int mh_sam2aln_conseq_ins(mh_ctx *ctx, char *buf, size_t cap, size_t *used);
/* The same text written to fd at offset with pwrite; *written = its size. */
int mh_sam2aln_conseq_ins_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written);
/* Per (reference, cutoff, pos) the sum of conseq_ins.csv's counts over the
 * strings, in the text's order: name_id as in mh_sam2aln_clip_counts,
 * cut_index indexes the call's q-cutoffs as they were given.  *n = rows;
 * arrays NULL: only *n. */
int mh_sam2aln_ins_counts(mh_ctx *ctx, int32_t *name_id, int32_t *cut_index, int64_t *pos,
                          int32_t *count, int64_t cap, int64_t *n);
/* What the last mh_sam2aln_write of aligned.csv (which 0, the only one kept)
 * wrote: the crc32 of its text, joined from the formatted pieces' own
 * (nothing is read back), and its size.  -3 when this context's sam2aln
 * results were not written that way since they were computed. */
int mh_sam2aln_written(mh_ctx *ctx, int which, uint32_t *crc, int64_t *bytes);
/* The number of calls that have rebuilt the context's sam2aln results so far
 * (mh_sam2aln_csv[_q], _file[_q], _resident, _part): equal serials mean the
 * results are those of the same call. */
int mh_sam2aln_serial(mh_ctx *ctx, int64_t *serial);
/* Of the last call of either kind: out[0] pairs, out[1] pairs merged on the
 * device, out[2] distinct (rname, q-cutoff, merged sequence), i.e. the data
 * rows of aligned.csv, out[3] failed pairs, i.e. the data rows of failed.csv. */
int mh_sam2aln_stats(mh_ctx *ctx, int64_t *out4);
/* Host wall time (ms) of the last call: [0] CSV parse + matchmaker (unit
 * building for mh_sam2aln_resident), [1] upload (the stage kernel for
 * mh_sam2aln_resident) + device merge/group + fetch, [2..4] formatting of
 * the three outputs (0 until formatted). */
int mh_sam2aln_timing(mh_ctx *ctx, double *ms5);

/* ---- sam2aln split over the ranks of a job (same reference call,
 * sam2aln.py:395-478; the bytes move between ranks through the caller's
 * collectives, torch.distributed in sam2aln._sam2aln_sharded).  Rank `part`
 * of `parts`:
 *   mh_sam2aln_part       parses its share of remap.csv (fd, mmap'd): the
 *                         record at or after byte part/parts of the body, a
 *                         cut between the two rows of one qname moved past
 *                         the second, and merges its pairs on its device.
 *                         0, or 1 = not split (a line with an odd number of
 *                         '"', no qname column, '\r' in the file: every rank
 *                         gets 1 and the caller runs mh_sam2aln_file on one).
 *                         info[0..5] = units, pair units, reference names,
 *                         distinct merged sequences, share bytes, file bytes.
 *   mh_sam2aln_part_units qname hash (n = info[0]) and leftover flag per
 *                         unit: the caller checks that no leftover qname
 *                         has rows on two ranks (matchmaker, :291-312, pairs
 *                         across the whole file), else falls back.
 *   mh_sam2aln_part_names this rank's reference names ('\n' after each) and
 *                         the first unit of each; _set_names gives each its
 *                         job-wide id (the names in first-appearance order,
 *                         the order of groups in aligned.csv, :449-478).
 *   mh_sam2aln_records    step 0: distinct sequences as records, one buffer
 *                         per owner rank (hash % parts), sizes[parts];
 *                         step 1: up to per_name evenly spaced records of
 *                         every name of the owner's merged order, sizes[1];
 *                         step 2 (after mh_sam2aln_splitters): the owner's
 *                         records to the rank of their range, sizes[parts].
 *                         *data = the concatenated buffers (valid until the
 *                         next call on ctx).
 *   mh_sam2aln_records_merge  stage 0: the records every rank sent this
 *                         owner, equal ones added up (:446-452), sorted as
 *                         aligned.csv lists them (:466-470); stage 1: the
 *                         records of this rank's ranges, sorted.
 *   mh_sam2aln_splitters  all ranks' samples -> the splitters of each name.
 *   mh_sam2aln_range_counts   rows of this rank's range per job-wide name.
 *   mh_sam2aln_range_text aligned.csv rows of this rank's range (:471-478),
 *                         one segment per name, row numbers ("rank" column)
 *                         from base[name] (the rows of ranks before it).
 *   mh_sam2aln_part_text  insert.csv (which 1) / failed.csv (which 2) rows
 *                         of this rank's pair units (seg 0) or leftover
 *                         units (seg 1), with the header when head != 0; the
 *                         caller writes segments segment-major by rank. */
int mh_sam2aln_part(mh_ctx *ctx, int fd, int part, int parts, int q_cutoff, double max_prop_n,
                    int64_t *info);
int mh_sam2aln_part_units(mh_ctx *ctx, uint64_t *qhash, uint8_t *leftover);
int mh_sam2aln_part_names(mh_ctx *ctx, char *buf, size_t cap, size_t *used, int64_t *first_unit);
int mh_sam2aln_part_set_names(mh_ctx *ctx, const int32_t *gid, int n);
int mh_sam2aln_records(mh_ctx *ctx, int step, int parts, int per_name, int64_t *sizes,
                       const uint8_t **data);
int mh_sam2aln_records_merge(mh_ctx *ctx, int stage, const uint8_t *data, int64_t len);
int mh_sam2aln_splitters(mh_ctx *ctx, const uint8_t *data, int64_t len, int parts);
int mh_sam2aln_range_counts(mh_ctx *ctx, int n_names, int64_t *counts);
int mh_sam2aln_range_text(mh_ctx *ctx, int n_names, const char *const *names, const int64_t *base,
                          int64_t *seg_bytes, const uint8_t **data);
int mh_sam2aln_part_text(mh_ctx *ctx, int which, int seg, int head, int64_t *bytes,
                         const uint8_t **data);

/* ---- censor: replaces censor_fastq.censor (censor_fastq.py:32-102) ---- */
/* One FASTQ file (src, gzip when src_gzip) censored on the device: bases /
 * qualities at the bad (tile, cycle) pairs (tiles[k], cycles[k]; negative
 * cycles = reverse reads) become 'N' / '#', a trailing run of bad cycles is
 * dropped as the reference drops it, header and '+' lines are kept
 * verbatim.  *base_count / *score_sum = number and sum (Phred) of all
 * quality characters, for the summary row (:94-102).  The censored file
 * (gzip when dst_gzip: independent deflate members, level 1) is then
 * copied out with mh_censor_output (buf NULL: *used = size). */
int mh_censor_fastq(mh_ctx *ctx, const uint8_t *src, int64_t len, int src_gzip, int n_bad,
                    const char *const *tiles, const int32_t *cycles, int dst_gzip,
                    int64_t *base_count, int64_t *score_sum);
/* The same on the text a staged FASTQ holds (mh_fastq_open_part: the whole
 * file, or a rank's block of records of a sharded job; gzip already
 * inflated).  The text is taken (the handle keeps an empty one).
 * *out_bytes = size of the censored output held for mh_censor_output /
 * mh_censor_write. */
int mh_censor_staged(mh_ctx *ctx, mh_fastq *fq, int n_bad, const char *const *tiles,
                     const int32_t *cycles, int dst_gzip, int64_t *out_bytes,
                     int64_t *base_count, int64_t *score_sum);
int mh_censor_output(mh_ctx *ctx, char *buf, size_t cap, size_t *used);
/* The held censored output written to fd at offset (pwrite; the descriptor's
 * own offset is not used); *written = its size.  The output is released. */
int mh_censor_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written);
/* mh_censor_staged, the output written to fd from offset (pwrite) while it
 * is made: each gzip member (or text block) as soon as it and those before
 * it are done; *written = bytes written.  Nothing is kept for
 * mh_censor_output / mh_censor_write.  Replaces the same censor_fastq.py:
 * 32-102 call as mh_censor_staged + mh_censor_write. */
int mh_censor_staged_write(mh_ctx *ctx, mh_fastq *fq, int n_bad, const char *const *tiles,
                           const int32_t *cycles, int dst_gzip, int fd, int64_t offset,
                           int64_t *written, int64_t *base_count, int64_t *score_sum);
/* Host wall ms of the last call: [0] gunzip + record split, [1] upload +
 * k_censor (+ k_trim, k_primer, k_primer3) + download, [2] rewrite + gzip. */
int mh_censor_timing(mh_ctx *ctx, double *ms3);
/* 3' adapter trimming inside the censor pass (micall_amd.trim_fastqs; the
 * step bin/micall:133 names and does not have).  The adapters hold for this
 * context's following mh_censor_fastq / mh_censor_staged /
 * mh_censor_staged_write calls; n1 = n2 = 0 clears them.  seqs1 (n1 of them)
 * apply to the records whose header says read 1, seqs2 to all others: 0 to
 * 8 adapters each, 3 to 64 bases of ACGT.  max_errors[i], i = 0..64, is the
 * number of errors allowed in a match of i adapter bases (0 <= max_errors[i]
 * < max(i, 1)); min_overlap >= 1 is the shortest adapter prefix accepted at
 * the read's end.  Anything else: -3 and a message.
 * After k_censor, k_trim compares each record's censored sequence line (its
 * kept length n; an 'N' matches nothing) with each adapter a of its
 * direction: c(i, j) = the smallest unit-cost edit distance between a[:i]
 * and any r[s:j], s(i, j) the smallest such s.  Candidates are (m, j) for
 * every j with c <= max_errors[m] and (i, n) for min_overlap <= i < m with
 * c <= max_errors[i]; the smallest s wins (then the smaller c, the larger i,
 * the lower adapter index) and the sequence and quality lines are cut to s.
 * base_count / score_sum keep their meaning.  A record that keeps more than
 * 65 535 bases fails the call (-3, the record named). */
int mh_censor_set_adapters(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                           const char *const *seqs2, int min_overlap, const int32_t *max_errors);
/* What the last censor call trimmed: reads[d * 8 + k] records won by adapter
 * k of direction d (0: read 1, 1: the others), bases[...] the bases they
 * lost.  16 entries each; zero after mh_censor_set_adapters. */
int mh_censor_trim_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases);
/* Anchored 5' primer trimming inside the censor pass (micall_amd.trim_fastqs):
 * an amplicon read begins with the PCR primer that made it.  The primers hold
 * for this context's following mh_censor_fastq / mh_censor_staged /
 * mh_censor_staged_write calls; n1 = n2 = 0 clears them.  seqs1 (n1 of them)
 * apply to the records whose header says read 1, seqs2 to all others: 0 to
 * 256 primers each, 8 to 64 bases of ACGT.  max_errors[i], i = 0..64, is the
 * number of errors allowed in a primer of i bases (0 <= max_errors[i] <
 * max(i, 1) and i + max_errors[i] <= 127).  Anything else: -3 and a message
 * that names the primer or the table entry.
 * After k_censor (and k_trim, if adapters are set), k_primer compares each
 * record's kept sequence line (n bases; an 'N' matches nothing) with each
 * primer p (m bases) of its direction: D(j) = the unit-cost edit distance
 * between all of p and r[0:j], j = 0..min(n, m + max_errors[m]).  (k, j) is
 * a candidate when D(j) <= max_errors[m]; the larger m - D wins (then the
 * smaller D, the larger j, the lower primer index k) and the record's
 * sequence line is written from j to its kept length, its quality line from
 * min(j, kept quality length).  A record cut to nothing stays as an empty
 * record.  base_count / score_sum keep their meaning; the read-length cap
 * of the adapters does not apply (only the first 127 bases are read). */
int mh_censor_set_primers(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                          const char *const *seqs2, const int32_t *max_errors);
/* What the last censor call trimmed: reads[d * 256 + k] records won by primer
 * k of direction d (0: read 1, 1: the others), bases[...] the bases they
 * lost at the front.  512 entries each; zero after mh_censor_set_primers. */
int mh_censor_primer_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases);
/* 3' primer trimming inside the censor pass (micall_amd.trim_fastqs): a read
 * of an insert shorter than itself runs into the reverse complement of its
 * mate's primer.  The primers hold for this context's following censor
 * calls; n1 = n2 = 0 clears them.  seqs1 / seqs2 as for mh_censor_set_primers
 * (0 to 256 primers each, 8 to 64 bases of ACGT), written as they read in
 * the read.  max_errors[i], i = 0..64, is the number of errors allowed in i
 * bases (0 <= max_errors[i] < max(i, 1)); min_overlap is 1 to 64.  Anything
 * else: -3 and a message that names the primer or the table entry.
 * After k_censor, k_trim and k_primer, k_primer3 compares x = r[lead:n] (n
 * the kept length, lead k_primer's or 0; an 'N' matches nothing) with each
 * primer p (m bases) of the record's direction, b being the bases cut from
 * the end.  Full candidates: 1 <= b <= len(x) with F(b) <= max_errors[m],
 * F(b) the least unit-cost edit distance between all of p and r[n-b:e] over
 * e in n-b..n.  Partial candidates: min_overlap <= b <= min(len(x), m - 1)
 * with G(b) <= max_errors[b], G(b) the least edit distance between p[:i] and
 * all of r[n-b:n] over i in 0..m.  With L = m and D = F for a full, L = b and
 * D = G for a partial candidate, the larger L - D wins, then the smaller D,
 * the larger b, the lower primer index; the kept sequence and quality
 * lengths are lowered to n - b.  A record cut to nothing stays as an empty
 * record.  base_count / score_sum keep their meaning.  A record that keeps
 * more than 65 535 bases fails the call as it does with adapters. */
int mh_censor_set_primers3(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                           const char *const *seqs2, int min_overlap, const int32_t *max_errors);
/* What the last censor call trimmed: reads[d * 256 + k] records won by 3'
 * primer k of direction d (0: read 1, 1: the others), bases[...] the bases
 * they lost at the end.  512 entries each; zero after mh_censor_set_primers3. */
int mh_censor_primer3_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases);

/* ---- aln2counts: replaces the per-read loops of aln2counts.py ---------- */
/* aligned.csv text (refname, qcut, count, offset, seq columns) read as
 * csv.DictReader reads it; consecutive rows with equal (refname, qcut) form a
 * group (itertools.groupby, aln2counts.py:884-887).  Every row is counted on
 * the device in the three reading frames of _count_reads (:147-169): per
 * codon the 21 amino acids of AMINO_ALPHABET and, per codon position, the
 * bases A C G T N - (an 'n' is not counted, :642-645), each counter with the
 * first row of its group that touched it (the Counter insertion order that
 * most_common() breaks ties by).  codon_chars = the translations of the 216
 * codons over A C G T N - (translation.py:40-142), index 36 c0 + 6 c1 + c2.
 * slot 0..3 selects one of four independent row tables of the context.
 * Rejects (-3) seq characters outside A C G T N - n, offsets outside
 * 0..2^28 and counts outside 0..2^32-1.  *n_groups = number of groups. */
int mh_a2c_load_csv(mh_ctx *ctx, int slot, const char *text, int64_t len,
                    const char *codon_chars, int64_t *n_groups);
/* mh_a2c_load_csv on the whole of a regular file (fd, mmap'd): 0, or 1 when
 * the file holds '\r' (the caller reads it in text mode instead). */
int mh_a2c_load_file(mh_ctx *ctx, int slot, int fd, const char *codon_chars, int64_t *n_groups);
/* The same table as mh_a2c_load_file on the aligned.csv of this context's
 * last sam2aln call, built on the device from that call's resident results
 * (nothing is formatted or parsed): the rows in aligned.csv's order
 * (k_a2c_stage), the bin lists (k_a2c_bin_count / k_a2c_bin_fill), then
 * k_a2c_count as for a file; the sequence bytes are copied into the slot, so
 * a later sam2aln call leaves it intact.  0, or 1 when the rows cannot stand
 * for the file and the caller loads the file instead: no complete un-sharded
 * sam2aln result in the context; a reference name holding '"', ',', '\r' or
 * '\n'; 2^31-1 rows or more, a group whose counts add up to more than 2^32-1,
 * an offset or length above 2^28; a sequence byte outside A C G T N - n.
 * Negative only for HIP / allocation failures. */
int mh_a2c_load_resident(mh_ctx *ctx, int slot, const char *codon_chars, int64_t *n_groups);
/* The same from rows in memory: row r's seq is pool[seq_off[r] ..
 * seq_off[r] + seq_len[r]); group g = rows group_first[g] ..
 * group_first[g + 1] - 1 (group names are empty). */
int mh_a2c_load_rows(mh_ctx *ctx, int slot, int64_t n_rows, const char *pool, int64_t pool_len,
                     const int64_t *seq_off, const int32_t *seq_len, const int64_t *offset,
                     const int64_t *count, int64_t n_groups, const int64_t *group_first,
                     const char *codon_chars);
/* info5 = first row, rows, and the SeedAmino list length of frames 0, 1, 2;
 * names = refname '\0' qcut (names NULL: only *used = bytes needed). */
int mh_a2c_group(mh_ctx *ctx, int slot, int64_t g, int64_t *info5, char *names, size_t cap,
                 size_t *used);
/* Counters of group g, frame 0..2, codons 0 .. info5[2 + frame] - 1:
 * aa_count / aa_first [codon][21], nuc_count / nuc_first [codon][3][6]
 * (position in the codon, base A C G T N -); first = 0xffffffff when never
 * touched (the Counter has no such key). */
int mh_a2c_counts(mh_ctx *ctx, int slot, int64_t g, int frame, uint32_t *aa_count,
                  uint32_t *aa_first, uint32_t *nuc_count, uint32_t *nuc_first);
/* The codons of group g, frame 0..2 that mh_a2c_counts' 21 letters leave out
 * because they translate to no amino acid: xpd [codon][3] = X (three of
 * A C G T N, ambiguous), partial ('-' or 'n' beside a base) and del (three
 * '-' of the read itself, not the padding around it), each the summed count
 * column of its rows; codons 0 .. info5[2 + frame] - 1.  A codon without any
 * base that is no deletion (padding, the gap between the mates) is counted
 * nowhere.  The first call after a load counts all groups and frames of the
 * slot in one launch (k_a2c_detail, over the rows and chunks the load left
 * on the device); later calls copy.  After mh_a2c_part_count the counters
 * are those of this rank's rows (the caller adds the ranks up).  -3 for a
 * slot without a load, a bad group or frame. */
int mh_a2c_codon_detail(mh_ctx *ctx, int slot, int64_t g, int frame, uint32_t *xpd);
/* InsertionWriter.write's read loop (:779-795) over the rows of group g for
 * the codon ranges [left[k], right[k]) in reading frame `frame`: distinct
 * amino-acid strings per range with their summed counts, in (range, first
 * row) order.  *n_entries = number of strings; fetch them with
 * mh_a2c_insert_entries (aminos: one string per line). */
int mh_a2c_inserts(mh_ctx *ctx, int slot, int64_t g, int frame, int n_ranges,
                   const int32_t *left, const int32_t *right, int64_t *n_entries);
int mh_a2c_insert_entries(mh_ctx *ctx, int slot, int32_t *range, int64_t *count,
                          uint32_t *first, char *aminos, size_t cap, size_t *used);
/* The insertion report rows (aln2counts InsertionWriter.write) of the last
 * mh_a2c_inserts: per entry, lead + (left[range] + 1) + ',' + its amino-acid
 * string + ',' + its count + ',' + target[range] (blank for INT32_MIN) +
 * eol.  buf NULL: formats and sets *used; then copies into buf. */
int mh_a2c_insert_rows(mh_ctx *ctx, int slot, const char *lead, int n_ranges, const int32_t *left,
                       const int32_t *target, const char *eol, char *buf, size_t cap, size_t *used);
/* Host wall ms: [0] parse of the last load, [1] its upload + k_a2c_count +
 * fetch, [2] mh_a2c_inserts since the last call of this function.  After
 * mh_a2c_load_resident: [0] the row order (when not built yet) + staging
 * (k_a2c_stage), [1] the bin lists + k_a2c_count + fetch. */
int mh_a2c_timing(mh_ctx *ctx, int slot, double *ms3);
/* The nucleotide variants of n_regions coordinate regions over the rows of
 * group g (the loop of aln2counts.py:346-375 and the report of :537-549): per
 * region k and row, clipped = ('-' * offset + seq)[start[k]:end[k]] (Python
 * slice rules) counts when twice its bytes other than '-' exceed ref_len[k];
 * equal clipped sequences (byte identity, the length included) add their
 * counts up (64-bit), and the region keeps its max_variants[k] greatest by
 * (count, sequence as bytes).  A region with max_variants 0 costs no device
 * work.  The cut, ties in count included, is decided on the device: besides
 * fixed-size records only the kept sequences' text comes to the host.
 * key_bits (8..64) = hash bits used as the grouping key: 64 in the product;
 * a small value makes distinct sequences share a key, which every call
 * detects (each row's window is compared with its entry's first row's) and
 * reports as -4 "variant hash collision", never as a merged count.
 * n_kept[k] (may be NULL) = entries kept for region k.  -3: a negative
 * window, reference length or cut, n_regions < 1, key_bits outside 8..64. */
int mh_a2c_variants(mh_ctx *ctx, int slot, int64_t g, int n_regions, const int64_t *start,
                    const int64_t *end, const int64_t *ref_len, const int64_t *max_variants,
                    int key_bits, int64_t *n_kept);
/* The kept entries of the last mh_a2c_variants in report order (region index,
 * then count and sequence descending): region, count, len per entry, and the
 * sequences back to back (padding '-' materialised) in seqs.  seqs NULL:
 * *used = bytes needed. */
int mh_a2c_variant_entries(mh_ctx *ctx, int slot, int32_t *region, int64_t *count, int32_t *len,
                           char *seqs, size_t cap, size_t *used);
/* Of the last mh_a2c_variants: stats4 = (region, row) pairs that counted,
 * distinct entries, entries sharing the last kept count of a region whose cut
 * left some of them out, bytes of sequence text copied to the host; *ms (may
 * be NULL) = host wall ms of the call, device work included. */
int mh_a2c_variant_stats(mh_ctx *ctx, int slot, int64_t *stats4, double *ms);
/* Linked amino acids (not in the reference): n_sets sets of consensus codons
 * over the rows of group g.  Set s holds the codons codon[set_first[s] ..
 * set_first[s + 1]) (1 to 12 of them, 0-based, in the order of the haplotype)
 * and is read in reading frame frame[s] (0..2); set_first[0] = 0.  A row's
 * codon at k is the bytes at read indices 3k - frame - offset + 0..2, '-'
 * outside the row, and its character is the class mh_a2c_counts /
 * mh_a2c_codon_detail count it in: one of the 21 letters, 'X', '?' (partial),
 * '-' (del).  A row counts for a set when none of the set's codons is blank
 * (padding only, or only the gap between the mates); its haplotype is the
 * set's characters, and equal haplotypes of a set add their counts up
 * (64-bit).  The grouping key is the haplotype itself (5 bits a codon, the
 * set's index within a pass of at most 16 sets and 64 codons in the top four
 * bits; further sets go in further passes), so there is no collision to
 * report.  Only entries with count >= min_count leave the device, as
 * fixed-size records; a set's coverage (mh_a2c_link_stats) is the summed
 * count of every row that counts for it, the rows of dropped entries
 * included.  A codon beyond the group's extent is legal: every row is blank
 * there.  After mh_a2c_part_count the rows are this rank's share.
 * *n_entries (may be NULL) = entries kept.  -3: n_sets < 1, a set of 0 or
 * more than 12 codons, a frame outside 0..2, a negative codon,
 * min_count < 1, a slot without a load, no group g. */
int mh_a2c_link(mh_ctx *ctx, int slot, int64_t g, int n_sets, const int32_t *set_first,
                const int32_t *frame, const int32_t *codon, int64_t min_count, int64_t *n_entries);
/* The entries of the last mh_a2c_link in report order (sets as given, then
 * count descending, then haplotype bytes ascending): set and count per entry,
 * and one haplotype per line in haplotypes.  haplotypes NULL: *used = bytes
 * needed. */
int mh_a2c_link_entries(mh_ctx *ctx, int slot, int32_t *set, int64_t *count, char *haplotypes,
                        size_t cap, size_t *used);
/* Of the last mh_a2c_link: coverage[s] (may be NULL) per set; stats3 = (set,
 * row) pairs that counted, distinct entries on the device, entries copied to
 * the host; *ms (may be NULL) = host wall ms of the call, device work
 * included. */
int mh_a2c_link_stats(mh_ctx *ctx, int slot, int64_t *coverage, int64_t *stats3, double *ms);
/* Pairwise covariation (not in the reference): the weighted Gram matrix of
 * n_cols (1 to 512) bit columns over the rows of group g.  Column i is read at
 * consensus codon codon[i] (0-based) in reading frame frame[i] (0..2) and
 * holds a row when the row's character there -- mh_a2c_link's, numbered 1..24
 * in the order ACDEFGHIKLMNPQRSTVWY*X?- with 0 for a blank codon -- has its
 * bit set in mask[i]: one bit for one character, 22 bits (the letters and
 * '-') for "called".  gram[i * n_cols + j] = the summed count of the rows that
 * columns i and j both hold: symmetric, returned in full, the diagonal a
 * column's own count; exact in 64 bits.  Every row is read once for all
 * columns (k_a2c_gram_bits: one bit per column and row, one classification
 * per distinct (frame, codon)); the pairs are popcounts over the planes of the
 * counts (k_a2c_gram_pairs).  A codon beyond the group's extent is legal:
 * zeros.  After mh_a2c_part_count the rows are this rank's share, and the
 * job's matrix is the sum of the ranks'.  -3: n_cols outside 1..512, a frame
 * outside 0..2, a negative codon, a mask that is 0 or has bit 0 or a bit
 * above 24 set, a slot without a load, no group g. */
int mh_a2c_gram(mh_ctx *ctx, int slot, int64_t g, int n_cols, const int32_t *frame,
                const int32_t *codon, const uint32_t *mask, int64_t *gram);
/* Of the last mh_a2c_gram (zeros after a load or a refused call): stats[5] =
 * rows of the group, 64-row words, planes of the counts that occur, distinct
 * (frame, codon) classified, 64 x 64 tiles of pairs computed; *ms (may be
 * NULL) = host wall ms of the call, device work included. */
int mh_a2c_gram_stats(mh_ctx *ctx, int slot, int64_t *stats, double *ms);

/* ---- aln2counts counting split over the ranks of a job (the same
 * aln2counts.py:115-172 loops; the counters are sums and a first row is a
 * minimum, so each rank counts its share and the caller reduces them) ----
 *   mh_a2c_part_open     rank `part` of `parts` parses the rows of its share
 *                        of aligned.csv (fd, mmap'd; cuts at line starts).
 *                        0, or 1 = not split (a quoted field in the share or
 *                        '\r' in the file: the caller loads it whole).
 *                        info3 = rows, local groups, share bytes.
 *   mh_a2c_part_groups   its runs of (refname, qcut): keys "refname\x1fqcut\n"
 *                        each (keys NULL: *used only), rows, the codon
 *                        extent of frames 0..2 (ncod3[3 g + f]) and the
 *                        summed count of each.
 *   mh_a2c_part_count    the job's groups (n_groups keys as above, the codon
 *                        extents the maximum over ranks), gid[k] = the job
 *                        group of local run k (increasing), row_base[k] = rows
 *                        of that group on the ranks before; counts on the
 *                        device.  *cells = counter cells (aa + nuc, all
 *                        groups and frames), as mh_a2c_counts lays them out.
 *   mh_a2c_part_counters set 0: copies the cells' counts and first rows out;
 *                        set 1: takes the reduced ones (counts summed, first
 *                        rows the minimum) back, after which mh_a2c_group /
 *                        mh_a2c_counts read the job's counters.
 *   mh_a2c_insert_export the entries of the last mh_a2c_inserts as bytes
 *                        (buf NULL: *used only);
 *   mh_a2c_insert_merge  every rank's exports of one call concatenated:
 *                        equal (range, string) added up, first row the least,
 *                        in (range, first row) order (InsertionWriter.write,
 *                        :779-795), for mh_a2c_insert_entries / _rows. */
int mh_a2c_part_open(mh_ctx *ctx, int slot, int fd, int part, int parts, const char *codon_chars,
                     int64_t *info3);
int mh_a2c_part_groups(mh_ctx *ctx, int slot, char *keys, size_t cap, size_t *used, int64_t *rows,
                       int32_t *ncod3, int64_t *total);
int mh_a2c_part_count(mh_ctx *ctx, int slot, int64_t n_groups, const char *keys, const int64_t *gid,
                      const int32_t *ncod3, const int64_t *row_base, int64_t *cells);
int mh_a2c_part_counters(mh_ctx *ctx, int slot, int set, uint32_t *cnt, uint32_t *first);
int mh_a2c_insert_export(mh_ctx *ctx, int slot, uint8_t *buf, size_t cap, size_t *used);
int mh_a2c_insert_merge(mh_ctx *ctx, int slot, const uint8_t *buf, int64_t len, int64_t *n_entries);

/* ---- Gotoh: replaces _gotoh2.align (_gotoh2.c:544-607) ---------------- */
/* seq1/seq2 already cleaned (gotoh2.py:70-72).  out1/out2 need
 * strlen(seq1)+strlen(seq2)+1 bytes (cap). */
int mh_gotoh_align(mh_ctx *ctx, const char *seq1, const char *seq2, int gop, int gep,
                   int is_global, const char *alphabet, const int *matrix, char *out1,
                   char *out2, int cap, int *score);

/* Many alignments with the same scoring in one launch (one workgroup each):
 * the consensus-distance filter's K x K alignments (remap.py:244-263) and
 * aln2counts' coordinate alignments.  status[t] = 0, or -1 where
 * _gotoh2.align would raise "Traceback failed"; the call itself returns
 * -3 / -2 / -4 for a bad argument / out of memory / a HIP error. */
int mh_gotoh_align_batch(mh_ctx *ctx, int count, const char *const *seq1,
                         const char *const *seq2, int gop, int gep, int is_global,
                         const char *alphabet, const int *matrix, char *const *out1,
                         char *const *out2, const int *cap, int *score, int *status);

/* The consensus-distance filter's edit distances (remap.py:247-251) as one
 * device batch: alignment t is mh_gotoh_align_batch's (seq1[t], seq2[t])
 * and dist[t] = Levenshtein.distance(extract_relevant_seed(aligned seq2,
 * aligned seq1), text[t]) (remap.py:129-138, :251), computed on the device
 * from the alignment (k_lev_prep, k_lev); only the distances are fetched.
 * status[t] = 0, -1 where the traceback fails, or -2 where the aligned
 * seq2 has no non-gap column (the reference's match is None); score[t] is
 * the alignment score.  Replaces remap.py:249-251's per-pair aligner.align +
 * extract_relevant_seed + Levenshtein.distance calls. */
int mh_gotoh_distance_batch(mh_ctx *ctx, int count, const char *const *seq1,
                            const char *const *seq2, const char *const *text, int gop, int gep,
                            int is_global, const char *alphabet, const int *matrix, int *dist,
                            int *score, int *status);

/* Per-kernel device time measured with HIP events on the context's stream
 * (k_seed, k_dp, k_pair, k_pileup).  mh_profile(ctx, 1) enables and resets. */
int mh_profile(mh_ctx *ctx, int enable);
int mh_profile_get(mh_ctx *ctx, const char *kernel, double *total_ms, int64_t *launches);

/* Diagnostics (tests only; no reference counterpart): for n caller-given
 * extensions items[4t..4t+3] = (read index, strand, ref, centre diagonal) of
 * the loaded reads against the built index, run both k_dp paths on the same
 * staged tables: out[8t..8t+7] = (fast path taken, its best score, row, band
 * lane; the band half; the full banded DP's best score, row, band lane).
 * Whenever the fast path is taken its cell must equal the full DP's. */
int mh_probe_extend(mh_ctx *ctx, const mh_params *par, int n, const int32_t *items, int32_t *out);

/* Host side of counts_to_conseqs (remap.py:309-333 with find_top_token
 * :892-902 and the seed prefill :195-197) for one reference's fetched
 * pileup rows, positions 1..length (rows past `rows` count as empty): tok[i]
 * = the top base-like token of position i+1 -- the first of A < C < G < T
 * with the largest positive count, else the seed's character (count 0),
 * else 'N' (-1), else '-' (-2), else 0 (no token).  Insertion tokens are
 * merged in by the caller.  *any_positive: some row holds a positive count.
 * Replaces the reference's per-position Counter walk. */
int mh_top_tokens(int32_t length, int32_t rows, const int32_t *dense, const uint8_t *nflag,
                  const uint8_t *dflag, const char *seed, int32_t seed_len, uint8_t *tok,
                  int32_t *any_positive);

/* counts_to_conseqs (remap.py:309-333, find_top_token :892-902, seed
 * prefill :195-197) for n_sel references of a fetched pileup in one call
 * (host code): reference k is row rows_of[k] of dense ([rows][cap][4]
 * int32) / nflag / dflag ([rows][cap] bytes), positions 1..lengths[k], its
 * seed seeds[k] (seed_lens[k] bytes, may be 0); the insertion tokens are
 * n_ev events (row, pos, token = pool[off .. off+len), merged pairs).  Per
 * position the top of the reference's Counter, then the deletion-run rule;
 * consensus k is out[out_off[k] .. out_off[k+1]) and present[k] = 0 when no
 * count is positive (no consensus).  out_cap >= sum(lengths) + sum(ev_len)
 * always suffices.  Returns -2 when out_cap is too small. */
int mh_conseqs_build(int n_sel, const int32_t *rows_of, const int32_t *lengths, const char *const *seeds,
                     const int32_t *seed_lens, int32_t cap, const int32_t *dense, const uint8_t *nflag,
                     const uint8_t *dflag, int64_t n_ev, const int32_t *ev_row, const int32_t *ev_pos,
                     const int64_t *ev_off, const int32_t *ev_len, const int64_t *ev_cnt, const char *pool,
                     char *out, int64_t out_cap, int64_t *out_off, int32_t *present);

/* Unit-cost edit distance (Levenshtein.distance, remap.py:251). */
int mh_levenshtein(const char *a, const char *b);
/* out[t] = mh_levenshtein(a[t], b[t]) for count pairs, on host threads. */
int mh_levenshtein_batch(int count, const char *const *a, const char *const *b, int *out);

#ifdef __cplusplus
}
#endif
#endif
