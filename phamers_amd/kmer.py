"""
kmer.py -- drop-in for the hot-path functions of PhaMers' scripts/kmer.py, executed
by hand-written HIP kernels on an MI355X through libphamers_hip.so.

Same names, argument meaning, defaults and return shapes as the reference:

    count_string(sequence, kmer_length, symbols=DNA, normalize=False)   scripts/kmer.py:32
    count(data, kmer_length, symbols=DNA, normalize=False)              scripts/kmer.py:82
    count_file(input_file, kmer_length, symbols=DNA, normalize=False)   scripts/kmer.py:114
    count_directory(directory, kmer_length, identifier='fna', ...)       scripts/kmer.py:143
    normalize_counts(counts)                                            scripts/kmer.py:209
    kmers(k, symbols=DNA), sequence_to_integers, get_kmer_index         scripts/kmer.py:183-251
    main()   `python -m phamers_amd.kmer <fasta | dir> <out.csv> -k K`     scripts/kmer.py:283-334

Every counting function takes a trailing ``both_strands=False`` (this project's own; `--both_strands` on the command
line): with it a row holds the k-mers of the sequence AND of its reverse complement -- the forward counts folded on the
device (phk_batch_fold_strands) -- so a contig counts the same whichever strand it was written on.

Scope notes: only 4-symbol alphabets run on the GPU (the reference's
integer-replacement branch with DNA/RNA); other alphabets raise NotImplementedError --
there is no CPU fallback in this package.
"""
import logging
import os
import random

import numpy as np

from . import _lib

logging.basicConfig(format='[%(asctime)s][%(levelname)s][%(funcName)s] - %(message)s')
logger = logging.getLogger(__name__)
logger.setLevel(logging.WARNING)

DNA = 'ATGC'
RNA = 'AUGC'
protein = 'RHKDESTNQCUGPAVILMFYW'


def _check_symbols(symbols):
    if len(symbols) != 4 or len(set(symbols)) != 4:
        raise NotImplementedError(
            "phamers_amd counts k-mers over 4-symbol alphabets (DNA/RNA) on the GPU; symbols=%r is "
            "outside the accelerated path (use PhaMers' own kmer.py for it)" % (symbols,))
    try:
        return symbols.encode('latin-1')
    except UnicodeEncodeError:
        raise NotImplementedError("symbols must be single-byte characters")


def _check_strands(symbols, both_strands):
    """The reverse complement pairs the symbols by their digit (0 <-> 1, 2 <-> 3): A <-> T(U), G <-> C for DNA / RNA only."""
    if both_strands and symbols not in (DNA, RNA):
        raise NotImplementedError("both_strands needs symbols 'ATGC' (DNA) or 'AUGC' (RNA), whose order pairs each base "
                                  "with its complement; got %r" % (symbols,))
    return bool(both_strands)


def _count_batch(sequences, kmer_length, symbols, both_strands=False):
    """n sequences -> (n, 4^k) int64 via phk_count_ascii (one upload, one launch chain); ``both_strands``: through a
    resident batch, folded on the device."""
    k = int(kmer_length)
    sym = _check_symbols(symbols)
    if _check_strands(symbols, both_strands):
        batch = _lib.Batch.from_sequences(_lib.get_context(), sequences, k, sym)
        try:
            return batch.fold_strands().counts()
        finally:
            batch.close()
    n = len(sequences)
    D = 4 ** k
    raw = [s.encode('latin-1', 'replace') for s in sequences]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    if n:
        offsets[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    bases = np.frombuffer(b''.join(raw) or b'\0', dtype=np.uint8)
    out = np.zeros((n, D), dtype=np.int64)
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_count_ascii(ctx.handle, _lib.ptr(np.ascontiguousarray(bases)), _lib.ptr(offsets),
                                       n, k, sym, _lib.ptr(out)))
    return out


def count_string(sequence, kmer_length, symbols=DNA, normalize=False, both_strands=False):
    """k-mer counting function (scripts/kmer.py:32-79): forward-strand, stride-1 windows;
    windows touching a character outside ``symbols`` (case-sensitive) are skipped; bin index
    has the first base as the most significant base-4 digit ('AAAT' -> 1).  Returns a 1-D
    int64 array of length 4^k, or float64 frequencies when ``normalize`` (all zeros stay
    zeros).  ``both_strands``: the sequence and its reverse complement counted together (the row sum doubles)."""
    counts = _count_batch([sequence], kmer_length, symbols, both_strands)[0]
    if normalize:
        counts = counts.astype(float)
        if np.sum(counts) > 0:
            counts = normalize_counts(counts)
    return counts


def count(data, kmer_length, symbols=DNA, normalize=False, both_strands=False):
    """K-mer counting dispatcher (scripts/kmer.py:82-111): str -> 1-D; list of one string ->
    1-D; list of n strings -> (n, 4^k); anything else -> None (logged)."""
    if isinstance(data, list):
        if len(data) == 1:
            return count(data[0], kmer_length, symbols=symbols, normalize=normalize, both_strands=both_strands)
        logger.info("Counting %d-mers in %d sequences..." % (kmer_length, len(data)))
        kmer_count = _count_batch(data, kmer_length, symbols, both_strands)
        if normalize:
            # per-row count_string(normalize=True): zero rows stay zero (scripts/kmer.py:77)
            sums = kmer_count.sum(axis=1)
            kmer_count = normalize_counts(kmer_count) if len(data) else kmer_count.astype(float)
            kmer_count[sums == 0] = 0.0
    elif isinstance(data, str):
        kmer_count = count_string(data, kmer_length, symbols=symbols, normalize=normalize, both_strands=both_strands)
    else:
        logger.info("Data was not str or list: %s\n%s ..." % (type(data), data.__str__()[:25]))
        kmer_count = None
    return kmer_count


def cut_plan(lengths, cut_size):
    """The pieces of ``count_cuts`` for sequences of the given lengths: (offsets, keep, owner, index).  Sequence r is cut at
    every ``cut_size`` bases from its start; ``offsets`` (uint64, pieces + 1) are the piece boundaries in the concatenated
    bases, tails included; ``keep`` = the pieces of exactly ``cut_size`` bases, by position; ``owner`` / ``index`` = the
    sequence each kept piece comes from and its number within it."""
    cut_size = int(cut_size)
    if cut_size < 1:
        raise ValueError("cut_size must be >= 1, got %r" % (cut_size,))
    lengths = np.asarray(lengths, dtype=np.int64)
    full = lengths // cut_size
    pieces = full + (lengths % cut_size != 0)                     # a shorter tail is one more piece
    first = np.concatenate(([0], np.cumsum(pieces)))              # first piece of every sequence
    starts = np.concatenate(([0], np.cumsum(lengths)))
    owner_all = np.repeat(np.arange(len(lengths)), pieces)
    index_all = np.arange(first[-1]) - first[owner_all]
    offsets = np.empty(first[-1] + 1, dtype=np.uint64)
    offsets[:-1] = starts[owner_all] + index_all * cut_size
    offsets[-1] = starts[-1]
    keep = np.flatnonzero(index_all < full[owner_all])
    return offsets, keep, owner_all[keep], index_all[keep]


def count_cuts(fasta_file_or_sequences, kmer_length, cut_size, symbols=DNA, both_strands=False):
    """k-mer counts of the consecutive, non-overlapping pieces of exactly ``cut_size`` bases of every sequence (a shorter
    tail is dropped, a sequence shorter than ``cut_size`` gives no row): (ids, counts (pieces, 4^k) int64), id
    ``<record id>_<piece index>``.  ``fasta_file_or_sequences``: a FASTA path (record id = Bio.SeqIO's record.id, the
    first word of the title line: any FASTA file can be cut, whatever its headers look like) or a list of strings (record
    ids '0', '1', ...).  The cut rule is this project's own: the reference reads cut
    files (scripts/cut_validator.py) but ships nothing that writes them.  All pieces, tails included, are the contigs of
    ONE device batch over the file's bases (phk_batch_from_ascii); phk_batch_select keeps the full-size ones.
    ``both_strands``: every piece with its reverse complement (the kept rows are folded on the device)."""
    import ctypes
    sym = _check_symbols(symbols)
    both_strands = _check_strands(symbols, both_strands)
    k = int(kmer_length)
    ctx = _lib.get_context()
    fasta = None
    if isinstance(fasta_file_or_sequences, str):
        fasta = _lib.Fasta(fasta_file_or_sequences)
    try:
        if fasta is not None:
            record_ids = fasta.ids()
            lengths, total = fasta.lengths(), fasta.total_bases
            bases_ptr, hold = ctypes.c_void_p(fasta._bases), None
        else:
            raw = [s.encode("latin-1", "replace") for s in fasta_file_or_sequences]
            record_ids = [str(i) for i in range(len(raw))]
            lengths, total = np.array([len(r) for r in raw], dtype=np.int64), sum(len(r) for r in raw)
            hold = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
            bases_ptr = _lib.ptr(np.ascontiguousarray(hold))
        offsets, keep, owner, index = cut_plan(lengths, cut_size)
        ids = ["%s_%d" % (record_ids[r], i) for r, i in zip(owner, index)]
        if len(keep) == 0:
            return ids, np.zeros((0, 4 ** k), dtype=np.int64)
        h = ctypes.c_void_p()
        _lib.check(ctx.lib.phk_batch_from_ascii(ctx.handle, bases_ptr, _lib.ptr(offsets), len(offsets) - 1, k, sym,
                                                ctypes.byref(h)))
        batch = _lib.Batch(ctx, h)
        try:
            chosen = batch.select(keep)
            try:
                if both_strands:
                    chosen.fold_strands()
                return ids, chosen.counts()
            finally:
                chosen.close()
        finally:
            batch.close()
    finally:
        if fasta is not None:
            fasta.close()


def window_plan(lengths, window, step):
    """The sliding windows of ``count_windows`` for sequences of the given lengths: (owner, start) as int64 arrays in row
    order.  Sequence r of length L >= ``window`` has the windows starting at ``j * step``, j = 0 .. (L - window) // step;
    rows are sequence-major and ordered by start; a shorter sequence has none."""
    window, step = int(window), int(step)
    if window < 1:
        raise ValueError("window must be >= 1, got %r" % (window,))
    if step < 1:
        raise ValueError("step must be >= 1, got %r" % (step,))
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    per = np.where(lengths >= window, (lengths - window) // step + 1, 0)
    first = np.concatenate(([0], np.cumsum(per))).astype(np.int64)
    owner = np.repeat(np.arange(len(lengths), dtype=np.int64), per)
    start = (np.arange(first[-1], dtype=np.int64) - first[owner]) * step
    return owner, start


def _windows_batch(fasta_file_or_sequences, kmer_length, window, step, symbols=DNA, _segment=0):
    """(record ids, lengths, device batch or None) of ``count_windows``: the windows of ``window_plan`` as the rows of one
    device-resident batch (phk_batch_windows_from_ascii / _from_fasta); None when there is no window at all.  The caller
    closes the batch."""
    sym = _check_symbols(symbols)
    k, window, step = int(kmer_length), int(window), int(step)
    if window < k:
        raise ValueError("window (%d) must be at least kmer_length (%d)" % (window, k))
    if step < 1:
        raise ValueError("step must be >= 1, got %r" % (step,))
    ctx = _lib.get_context()
    if isinstance(fasta_file_or_sequences, str):
        fasta = _lib.Fasta(fasta_file_or_sequences)
        try:
            record_ids, lengths = fasta.ids(), fasta.lengths()
            if not (lengths >= window).any():
                return record_ids, lengths, None
            return record_ids, lengths, _lib.Batch.windows_from_fasta(ctx, fasta, k, window, step, sym, _segment)
        finally:
            fasta.close()
    sequences = list(fasta_file_or_sequences)
    record_ids = [str(i) for i in range(len(sequences))]
    lengths = np.array([len(s) for s in sequences], dtype=np.int64)
    if not (lengths >= window).any():
        return record_ids, lengths, None
    return record_ids, lengths, _lib.Batch.windows_from_sequences(ctx, sequences, k, window, step, sym, _segment)


def count_windows(fasta_file_or_sequences, kmer_length, window, step, symbols=DNA, _segment=0, both_strands=False):
    """k-mer counts of the overlapping windows of ``window`` bases every ``step`` bases along every sequence
    (``window_plan``): (ids, counts (n_windows, 4^k) int64), id ``<record id>_<0-based start>``; row j of a sequence is
    what ``count_string(seq[j * step : j * step + window], k)`` returns.  Input kinds, alphabet and k rules are those of
    ``count_cuts``.  Every base goes to the device once, whatever the overlap: the kernel adds the k-mers entering a
    window and subtracts those leaving it.  ``_segment``: windows per work unit of that kernel
    (0 = chosen by the launch; the result does not depend on it).  ``both_strands``: every window with its reverse
    complement (the window rows are folded on the device).  ValueError for ``window < kmer_length`` or ``step < 1``."""
    both_strands = _check_strands(symbols, both_strands)
    record_ids, lengths, batch = _windows_batch(fasta_file_or_sequences, kmer_length, window, step, symbols, _segment)
    owner, start = window_plan(lengths, window, step)
    ids = ["%s_%d" % (record_ids[r], s) for r, s in zip(owner, start)]
    if batch is None:
        return ids, np.zeros((0, 4 ** int(kmer_length)), dtype=np.int64)
    try:
        if both_strands:
            batch.fold_strands()
        return ids, batch.counts()
    finally:
        batch.close()


def count_file(input_file, kmer_length, symbols=DNA, normalize=False, both_strands=False):
    """Counts k-mers of every record of a FASTA file (scripts/kmer.py:114-140).  Returns
    (ids, counts): ids parsed by the reference's header rules (scripts/id_parser.py:89-100),
    counts (n, 4^k).  An unreadable file gives (None, None).  The file is parsed once by the
    native multi-threaded reader (phk_fasta_read; plain or .gz) and counted on the GPU.  ``both_strands``: every record
    with its reverse complement."""
    sym = _check_symbols(symbols)
    both_strands = _check_strands(symbols, both_strands)
    try:
        fasta = _lib.Fasta(input_file)
    except IOError:
        logger.warning("Could not read file: %s" % os.path.basename(input_file))
        return None, None
    try:
        ids = fasta.phamers_ids()
        counts = np.zeros((len(ids), pow(len(symbols), kmer_length)), dtype=(int, float)[normalize])
        if fasta.n_records:
            # bases up once, counts down once (device-resident batch)
            batch = _lib.Batch.from_fasta(_lib.get_context(), fasta, kmer_length, sym)
            try:
                if both_strands:
                    batch.fold_strands()
                got = batch.counts()
                if normalize:
                    sums = got.sum(axis=1)
                    got = batch.normalized()
                    got[sums == 0] = 0.0
            finally:
                batch.close()
            counts[:, :] = got
    finally:
        fasta.close()
    return ids, counts


def count_directory(directory, kmer_length, identifier='fna', symbols=DNA, sum_file=True, sample=0, both_strands=False):
    """Counts k-mers of all FASTA files of a directory whose base name contains `identifier`
    (scripts/kmer.py:143-181): one row per file -- with sum_file the column sums over the file's records,
    labelled with the id of its first record (how the reference matrix is regenerated from genome files) --
    as a float array like the reference's.  Unreadable / empty / all-zero files are skipped with a warning;
    `sample` > 0 shuffles the files and stops after that many rows.  ``both_strands``: every record with its reverse
    complement (folded on the device before the column sums)."""
    selected_files = [os.path.join(directory, f) for f in os.listdir(directory) if identifier in os.path.basename(f)]
    if sample:
        random.shuffle(selected_files)
    ids, rows = [], []
    sym = _check_symbols(symbols)
    both_strands = _check_strands(symbols, both_strands)
    for path in selected_files:
        # one file = one device-resident batch; with sum_file its column sums are reduced on the device
        # (phk_batch_column_sums) and only the 4^k sums come back -- the per-record count matrix never does
        try:
            fasta = _lib.Fasta(path)
        except IOError:
            logger.warning("Could not read file: %s" % os.path.basename(path))
            continue
        try:
            file_ids = fasta.phamers_ids()
            if fasta.n_records == 0:
                logger.warning("Could not read file: %s" % os.path.basename(path))
                continue
            batch = _lib.Batch.from_fasta(_lib.get_context(), fasta, kmer_length, sym)
        finally:
            fasta.close()
        try:
            if both_strands:
                batch.fold_strands()
            if sum_file:
                file_counts = batch.column_sums()
            elif batch.n == 1:
                file_counts = batch.counts()[0]
            else:
                raise ValueError("count_directory(sum_file=False) needs single-record files (%s has %d records)"
                                 % (os.path.basename(path), batch.n))
        finally:
            batch.close()
        if np.sum(file_counts) == 0:
            logger.warning("Could not read file: %s" % os.path.basename(path))
            continue
        ids.append(file_ids[0])
        rows.append(file_counts)
        if sample and len(ids) == sample:
            break
    counts = np.zeros((len(rows), pow(len(symbols), kmer_length)))
    for i, r in enumerate(rows):
        counts[i] = r
    return ids, counts


def read_fasta(fasta_file):
    """(ids, sequences) of a FASTA file (scripts/fileIO.py:28-42), through the native reader."""
    fasta = _lib.Fasta(fasta_file)
    try:
        return fasta.phamers_ids(), fasta.sequences()
    finally:
        fasta.close()


def fasta_lengths(fasta_file):
    """(ids, sequence lengths): what phamer_scorer.screen_by_length needs (scripts/phamer.py:144-157)
    without materialising the sequences as Python strings."""
    fasta = _lib.Fasta(fasta_file, index_only=True)
    try:
        return fasta.phamers_ids(), fasta.lengths()
    finally:
        fasta.close()


def normalize_counts(counts):
    """Row-normalise a count array (scripts/kmer.py:209-221): float64 copy, each row divided
    by its sum; a zero row becomes NaN, exactly as in the reference."""
    counts = np.asarray(counts)
    shape = counts.shape
    if counts.ndim not in (1, 2):
        raise ValueError("normalize_counts expects a 1-D or 2-D array")
    rows = counts.reshape(1, -1) if counts.ndim == 1 else counts
    n, D = rows.shape
    out = np.empty((n, D), dtype=np.float64)
    if n == 0 or D == 0:
        return out.reshape(shape)
    ctx = _lib.get_context()
    if np.issubdtype(rows.dtype, np.integer) or rows.dtype == np.bool_:
        src = np.ascontiguousarray(rows, dtype=np.int64)
        _lib.check(ctx.lib.phk_normalize_i64(ctx.handle, _lib.ptr(src), n, D, _lib.ptr(out)))
    else:
        src = np.ascontiguousarray(rows, dtype=np.float64)
        _lib.check(ctx.lib.phk_normalize_f64(ctx.handle, _lib.ptr(src), n, D, _lib.ptr(out)))
    return out.reshape(shape)


# ---- label utilities (host-side strings; not arithmetic) ---------------------------------
def sequence_to_integers(sequence, symbols):
    """scripts/kmer.py:183-196: non-symbol characters -> '-', symbol i -> str(i)."""
    table = {s: str(i) for i, s in enumerate(symbols)}
    return ''.join(table.get(ch, '-') for ch in sequence)


def get_kmer_index(kmer, symbols):
    """scripts/kmer.py:199-206 (NB the reference parses in base len(kmer), right only when
    k == len(symbols); reproduced as is)."""
    return int(sequence_to_integers(kmer, symbols), len(kmer))


def kmers(k, symbols=DNA):
    """All k-mers in bin order (scripts/kmer.py:224-251)."""
    mers = ['']
    for _ in range(k):
        mers = [m + s for m in mers for s in symbols]
    return mers


def _parser():
    """The counting command line of scripts/kmer.py:283-303 (how the reference's data/reference_features CSVs were made:
    their '#' headers echo this Namespace): positional input (a FASTA file, or a directory of genome files) and output
    CSV; -k, -s / --sample, -sym / --symbols, -id / --file_identifier, -v, --debug."""
    import argparse
    ap = argparse.ArgumentParser(description="This script counts k-mers in sequence data",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('input_file', type=str, help='FASTA file, or a directory of FASTA files (one output row per file)')
    ap.add_argument('-id', '--file_identifier', type=str, default='.fna', help='File identifier if directory')
    ap.add_argument('output_file', type=str, help='Output CSV file of k-mer counts')
    ap.add_argument('-k', '--kmer_length', type=int, default=4, help='Length of k-mer to count')
    ap.add_argument('-s', '--sample', type=int, help='Number of sequences to sample and count')
    ap.add_argument('-sym', '--symbols', type=str, default=DNA, help='Symbols to use in k-mer counting')
    ap.add_argument('--both_strands', action='store_true', help='Count every sequence together with its reverse complement')
    ap.add_argument('-v', '--verbose', action='store_true', help='verbose output')
    ap.add_argument('--debug', action='store_true', help='Debug console')
    return ap


def main(argv=None):
    """`python -m phamers_amd.kmer <input> <output.csv> [-k K]` (scripts/kmer.py:283-334): a file goes through
    count_file, a directory through count_directory (column sums per file, reduced on the device); the result is
    written by fileIO.save_counts with the Namespace stamped into the '#' header, as the reference does."""
    from . import fileIO
    args = _parser().parse_args(argv)
    logger.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)
    logger.info("Counting k-mers...")
    if args.input_file and os.path.isfile(args.input_file):
        ids, counts = count_file(args.input_file, args.kmer_length, symbols=args.symbols, both_strands=args.both_strands)
        if ids is None:
            raise SystemExit(1)
    elif args.input_file and os.path.isdir(args.input_file):
        ids, counts = count_directory(args.input_file, args.kmer_length, symbols=args.symbols,
                                      identifier=args.file_identifier, sample=args.sample or 0,
                                      both_strands=args.both_strands)
    else:
        logger.error("%s was not an acceptable file or directory" % args.input_file)
        raise SystemExit(1)
    fileIO.save_counts(counts, ids, args.output_file, args=args)
    logger.info("K-mer counting complete.")
    return ids, counts


if __name__ == '__main__':
    main()
