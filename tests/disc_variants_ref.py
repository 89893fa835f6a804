"""Discovery behind its second pass, restated in plain Python from the reference's text: the variant records of
streamlined_discovery (src/typer/caller.cpp:2985-3092), Variant::add_base_in_front (src/typer/variant.cpp:1135-1167) over
Graph::get_generated_reference_genome (src/graph/graph.cpp:409-435), the order of Vcf::write_records (src/typer/vcf.cpp:1161-1275)
with its ID suffixes, and the text Vcf::write_record makes of a record without samples (:767-1015).

An event is (pos, type, seq): a 0-based contig position, 'X' / 'I' / 'D' and its letters (str).  The haplotype map is a list of
(event, ever, always) in the map's order (event_order), the two sets holding events; the indel table is {event: good}, `good` being
has_indel_good_support when the second pass is through.  A record is a dict(pos [0-based contig position of REF's first base],
type, ref, alt, gt_id, hap [ids], anti [ids]).  Everything is integers and letters; nothing here is shared with the library."""
import functools

BUCKET_SIZE = 50  # caller.cpp:2764
MAX_ALLELE_LETTERS = 16000  # vcf.cpp:797


def event_order(e):
    """Event::operator< (src/typer/event.cpp:198-207): position; insertions, deletions, SNPs; the sequence"""
    pos, kind, seq = e
    return (pos, {"I": 0, "D": 1, "X": 2}[kind], seq)


def generated_reference(reference, region_begin, begin, end):
    """Graph::get_generated_reference_genome (graph.cpp:409-435) over a reference-only graph of the region: 1-based contig positions
    [begin, end) -> (the letters, begin and end as the function leaves them: they are references)"""
    abs_first_from = region_begin + 1  # :412-413
    begin = max(abs_first_from, begin)  # :415
    end = min(abs_first_from + len(reference), end)  # :416
    if end < begin:  # :418-432
        return "", begin, end
    return reference[begin - abs_first_from:end - abs_first_from], begin, end  # :434


def add_base_in_front(reference, region_begin, pos, seqs, add_n=True):
    """variant.cpp:1135-1167 for a variant whose 0-based contig position is pos -> (True, new pos, new seqs) or (False, pos, seqs)"""
    contig_pos = pos + 1  # :1137 (abs_pos = event.pos + the offset of contig position 1, caller.cpp:2760, :3002)
    new_contig_pos = contig_pos - 1  # :1139
    first_base, got_begin, got_end = generated_reference(reference, region_begin, new_contig_pos, contig_pos)  # :1140
    if len(first_base) != 1 or got_end != contig_pos or got_begin != contig_pos - 1:  # :1142
        return False, pos, seqs
    base = first_base
    not_acgt = base not in "ACGT"  # :1145
    if not add_n and not_acgt:  # :1147
        return False, pos, seqs
    if add_n and not_acgt:  # :1150
        base = "N"
    seqs = [base + s if (len(s) == 0 or len(s) > 1 or s[0] != "*") else s for s in seqs]  # :1154-1161
    return True, pos - 1, seqs  # :1164


def records(reference, region_begin, table, haplotypes):
    """caller.cpp:2985-3092.  table: {event: good}; haplotypes: [(event, ever, always)] in the map's order"""
    def dropped(e):  # :2992-2999, :3050-3057
        return e[1] != "X" and not table.get(e, False)

    out = []
    for index, (event, ever, always) in enumerate(haplotypes):
        event_index = index + 1  # :2985, :2987
        if dropped(event):
            continue
        pos, kind, seq = event
        if kind == "X":  # :3009-3014
            assert 0 <= pos - region_begin < len(reference)  # :3006-3007
            seqs = [reference[pos - region_begin], seq]
        elif kind == "I":  # :3015-3021
            _, pos, seqs = add_base_in_front(reference, region_begin, pos, ["", seq])
        else:  # :3022-3028
            _, pos, seqs = add_base_in_front(reference, region_begin, pos, [seq, ""])
        hap, anti = [], []
        next_event_index = event_index + 1  # :3039
        for nxt, _, _ in haplotypes[index + 1:]:  # :3042
            if nxt[0] >= event[0] + 2 * BUCKET_SIZE:  # :3046
                break
            if not dropped(nxt):
                if nxt in always:  # :3060
                    hap.append(next_event_index)
                elif nxt not in ever:  # :3070
                    anti.append(next_event_index)
            next_event_index += 1
        out.append(dict(pos=pos, type=kind, ref=seqs[0], alt=seqs[1], gt_id=event_index, hap=hap, anti=anti))
    return out


def variant_type(seqs):
    """Variant::determine_variant_type (variant.cpp:1430-1520) for alleles of plain letters, NDEBUG (an empty allele passes)"""
    num_non_ones = sum(1 for s in seqs if len(s) > 1)  # :1455, :1479
    if num_non_ones == 0:  # :1509
        return "SG"
    if len(seqs) - num_non_ones == 1:  # :1512
        return "IG"
    if len(seqs) - num_non_ones == 2 and seqs[-1] == "*":  # :1515
        return "IG"
    return "XG"


def n_infos(r):
    return 1 + bool(r["hap"]) + bool(r["anti"])  # :3082-3088


def compare_variants(a, b):
    """vcf.cpp:1174-1214 -> True when a goes in front of b"""
    if a["pos"] != b["pos"]:  # :1183-1187
        return a["pos"] < b["pos"]
    order_a = int(a["type"] == "I") + 2 * int(a["type"] == "D")  # :1190-1197
    order_b = int(b["type"] == "I") + 2 * int(b["type"] == "D")
    if order_a != order_b:
        return order_a < order_b
    a_vt = int(len(a["ref"]) > len(a["alt"])) + 2 * int(len(a["ref"]) == len(a["alt"]))  # :1201-1210
    b_vt = int(len(b["ref"]) > len(b["alt"])) + 2 * int(len(b["ref"]) == len(b["alt"]))
    if a_vt != b_vt:
        return a_vt < b_vt
    sa, sb = [a["ref"], a["alt"]], [b["ref"], b["alt"]]
    return sa < sb or (sa == sb and n_infos(a) > n_infos(b))  # :1213


def sort_order(recs):
    """:1222-1227: the records' indices in the order they are written (no two records of a region are equal under compare_variants;
    a stable sort where they are)"""
    key = functools.cmp_to_key(lambda i, j: -1 if compare_variants(recs[i], recs[j]) else (1 if compare_variants(recs[j], recs[i]) else 0))
    return sorted(range(len(recs)), key=key)


def id_suffixes(recs, order):
    """:1231-1274 with the region of Vcf::write(".") -> per place in `order` the suffix, or None for a duplicate that is not written"""
    out = []
    dup = -1  # :1238
    for i, index in enumerate(order):
        if i == 0:
            out.append("")  # :1232-1235
            continue
        prev, cur = recs[order[i - 1]], recs[index]
        if (cur["pos"], cur["ref"], cur["alt"]) == (prev["pos"], prev["ref"], prev["alt"]):  # :1259, Variant::operator== variant.cpp:2242-2245
            out.append(None)
            continue
        if not (cur["pos"] == prev["pos"] and variant_type([cur["ref"], cur["alt"]]) == variant_type([prev["ref"], prev["alt"]])):  # :1216-1217, :1263
            out.append("")
            dup = -1
        else:
            dup += 1  # :1270
            out.append("." + str(dup))
    return out


def record_text(contig, r, suffix):
    """vcf.cpp:767-1015 for a record without calls in a file without samples -> its line, or "" when it is left out"""
    if len(r["ref"]) + len(r["alt"]) > MAX_ALLELE_LETTERS:  # :791-807
        return ""
    pos = r["pos"] + 1
    infos = {"GT_ID": str(r["gt_id"])}  # caller.cpp:3082-3088
    if r["hap"]:
        infos["GT_HAPLOTYPE"] = ",".join(map(str, r["hap"]))
    if r["anti"]:
        infos["GT_ANTI_HAPLOTYPE"] = ",".join(map(str, r["anti"]))
    info = ";".join("%s=%s" % (k, infos[k]) for k in sorted(infos))  # :994-1015, std::map's order
    return "%s\t%d\t%s:%d:%s%s\t%s\t%s\t0\t.\t%s\n" % (contig, pos, contig, pos, variant_type([r["ref"], r["alt"]]), suffix, r["ref"], r["alt"], info)  # :834-862


COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"  # (the last line of the header, vcf.cpp:693-762 without samples)


def sites_text(contig, recs):
    order = sort_order(recs)
    return COLUMNS + "".join(record_text(contig, recs[i], s) for i, s in zip(order, id_suffixes(recs, order)) if s is not None)
