"""A plain restatement of the walk over a read's CIGAR that starts discovery, written character by character from the
reference's text (run_first_pass, src/typer/caller.cpp:517-561, 583-793, 824-834).  Strings and lists only: it knows nothing of
bit planes, masks or groups of 32 bases, nor of a 16-bit length -- a deletion of any length that the reference makes an event of
is an event here (the product and oracle/gto_discovery.hpp state a limit there; the tests compare under that one exception).

It is the second statement beside oracle/gto_discovery.hpp; tests/test_disc_events_emu.py holds both to each other.

    walk(reference, region_begin, pos, cigar, sequence, qual) -> (state, pos_end, [events in CIGAR order])

reference: the region's bytes as a str, one character per byte (any byte may occur); pos: core.pos; cigar: the raw BAM words;
sequence: the read's bases as seq_nt16_str writes them (l_qseq characters of "=ACMGRSVTWYHKDBN"); qual: l_qseq base qualities.
An event is a dict with every field of gtx_disc_event but `read`: pos, seq, len, type (a character), hq, max_distance, reserved.
pos_end is relative to the region (what cov_down is indexed with); it is 0 for a read the pass does not walk."""

SKIPPED, COUNTED, END = 0, 1, 2
CIGAR_MAP = ['M', 'I', 'D', 'N', 'S', 'H', 'P', '=', 'X', 'B', '*', '*', '*', '*', '*', '*']  # caller.cpp:526-527
ACGT = ('A', 'C', 'G', 'T')


def walk(reference, region_begin, pos, cigar, sequence, qual):
    ref_size = len(reference)
    # :515 a read without a cigar or in front of the region is passed over
    if len(cigar) == 0 or pos < region_begin:
        return SKIPPED, 0, []
    read_offset = 0
    ref_offset = pos - region_begin  # :538
    if ref_offset >= ref_size:       # :550-560 the pass ends here
        return END, 0, []
    l_qseq = len(sequence)
    events = []
    for word in cigar:               # :583
        cigar_count = word >> 4
        operation = CIGAR_MAP[word & 15]
        if ref_offset >= ref_size:   # :592
            break
        if operation in ('M', '=', 'X'):  # :597-599
            for r in range(cigar_count):
                ref_pos = ref_offset + r
                if ref_pos >= ref_size:   # :605
                    break
                ref = reference[ref_pos]
                read_pos = read_offset + r
                if read_pos >= l_qseq:    # :611
                    break
                read_base = sequence[read_pos]
                if read_base == ref or ref not in ACGT or read_base not in ACGT:  # :617-621
                    continue
                events.append(dict(pos=ref_pos + region_begin, seq=ord(read_base), len=1, type='X', hq=1 if qual[read_pos] >= 25 else 0,  # :623, :647
                                   max_distance=min(read_pos, l_qseq - 1 - read_pos), reserved=0))  # :680
            read_offset += cigar_count
            ref_offset += cigar_count
        elif operation == 'I':       # :694
            begin = read_offset if read_offset < l_qseq else l_qseq                              # :698
            end = read_offset + cigar_count if read_offset + cigar_count < l_qseq else l_qseq   # :701
            if begin == end:         # :705 (the read offset stays)
                continue
            inserted = sequence[begin:end]
            if all(c in ACGT for c in inserted):  # :709
                events.append(dict(pos=region_begin + ref_offset, seq=begin, len=len(inserted), type='I', hq=1, max_distance=0, reserved=0))
            read_offset += cigar_count
        elif operation == 'D':       # :744
            if ref_offset + cigar_count >= ref_size:  # :748
                ref_offset += cigar_count
                continue
            deleted = reference[ref_offset:ref_offset + cigar_count]  # make_deletion_event: all of its bases
            if all(c in ACGT for c in deleted):       # :756
                events.append(dict(pos=region_begin + ref_offset, seq=ref_offset, len=len(deleted), type='D', hq=1, max_distance=0, reserved=0))
            ref_offset += cigar_count
        elif operation == 'S':       # :788
            read_offset += cigar_count
        # (:792 anything else moves neither the reference nor the read)
    return COUNTED, min(ref_offset, ref_size - 1), events  # :842
