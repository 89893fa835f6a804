"""The tables of the position-hinted pass (gtx_ctx_hint_table 0..6) restated in plain Python / numpy over the ORACLE's index.

Written from the comments of gtx_flat.hpp (IndexView: refp, pos_flags, filt, tail_info, the allele windows, the HINT_* constants) and from
the reference's lookup rule, not from index_build.hpp: the library's index, its half-key groups and its label records are not looked at.

  * the index is Oracle.index_dump(): keys ascending, labels (start, end, variant_id);
  * the graph is Oracle.graph(); the offsets of the nodes' bases, which that dump lacks, and the characters they point into come from the
    library's graph dict (tests/test_host_parity.py and tests/test_constructor_vectors.py hold that dict to the oracle's constructor);
  * a label's (site, allele) comes from its variant_id: the site is the reference node r whose [ref_first_var, ref_first_var + ref_nvar)
    holds it, the allele its offset in there;
  * the Hamming-1 neighbours of a key are found the reference's way: its 96 one-base variants, each looked up in the sorted keys;
  * "the keys that share K's first / last 16 bases" is a grouping on key >> 32 / key & 0xFFFFFFFF;
  * the special positions of a window's path are looked up in the oracle's (ref_reach_poses, actual_poses) table.

The library's own conservative limits are part of the definition (gtx_flat.hpp):
  * HINT_HE_CAP = 16: a verdict (HINT_EXACT_OK, the alleles' verdicts of HINT_ALT_OK) needs at most 16 keys in either half group of the key;
  * HINT_NB_MAX = 16: ... and its Hamming-1 neighbours at most 16 labels together;
  * a half group of more than 64 keys is not looked through: far code 0 (and no verdict -- HINT_HE_CAP says so sooner);
  * HINT_OWN_MAX = 4 labels of one k-mer, allele numbers below HINT_MASK_BITS = 8 for HINT_MULTI, below 4 for HINT_TWO;
  * windows for alleles of 1..HINT_WIN_ALLELE_MAX = 64 bases at sites of at most 8 alleles whose reference allele has 1..64 bases;
  * room, back and the next node's length are capped at 255; a site index has to fit the 16-bit field (below HINT_NO_SITE).

What the comments leave open and this file fixes (each is the narrow reading: a flag less, never one more):
  * the far codes, like every other field about K_i, speak of an INDEXED K_i: where the k-mer is in no key the field is 0;
  * the site field of x is HINT_NO_SITE wherever no flag names a site, k-mers that are not plain A/C/G/T included;
  * a window position whose k-mer does not reach into the allele carries the flag words of the linear reference's position that has those
    bases -- also in the last 32 places before the window's planes stop, where the linear reference goes on and the window does not;
  * the flags of the last 31 window positions (local + 32 > 384) are "none": the k-mer would leave the window.
"""
import numpy as np

K = 32
INVALID = 0xFFFFFFFF
SPECIAL_START = 0xD0000000
M32 = np.uint64(0xFFFFFFFF)

WIN_BEFORE, WIN_ALLELE_MAX, WIN_STRIDE = 160, 64, 384
EXACT_OK, SINGLE_OK, L1, R1, PAR, ALT_OK, MULTI, TWO = 1, 2, 4, 8, 16, 32, 64, 128
OWN_MAX, MASK_BITS = 4, 8
ALTIDX_SHIFT, SITE_SHIFT, NO_SITE = 8, 16, 0xFFFF
BACK_SHIFT, SNPOFF_SHIFT = 8, 16
SNP_GROUP, REFB_SHIFT, NV_SHIFT = 1 << 21, 22, 24
FAR_LEFT_SHIFT, FAR_RIGHT_SHIFT = 27, 29
NEAR_FREE = 1 << 31
TAIL_OK, TAIL_NODE, TAIL_NALL_SHIFT, TAIL_NEXT_SHIFT, TAIL_CODES_SHIFT = 1, 2, 2, 8, 16
HE_CAP, NB_MAX, GROUP_LOOK_MAX = 16, 16, 64
WINDOWS_MAX = 16384  # (GTX_HINT_WINDOWS' default)

IUPAC = "=ACMGRSVTWYHKDBN"  # a letter's 4-bit code is its place here
_NIBBLE = np.zeros(256, np.uint8)  # anything that is no IUPAC letter: 0, equal to no read base
for _i, _c in enumerate(IUPAC):
    _NIBBLE[ord(_c)] = _i
_TWO_OF = {1: 0, 2: 1, 4: 2, 8: 3}

X_FIELDS = [("EXACT_OK", 0, 1), ("SINGLE_OK", 1, 1), ("L1", 2, 1), ("R1", 3, 1), ("PAR", 4, 1), ("ALT_OK", 5, 1), ("MULTI", 6, 1), ("TWO", 7, 1),
            ("alleles", 8, 8), ("site", 16, 16)]
Y_FIELDS = [("room", 0, 8), ("back", 8, 8), ("snp_offset", 16, 5), ("SNP_GROUP", 21, 1), ("REFB", 22, 2), ("NV", 24, 3), ("far_left", 27, 2),
            ("far_right", 29, 2), ("NEAR_FREE", 31, 1)]
TAIL_X_FIELDS = [("TAIL_OK", 0, 1), ("TAIL_NODE", 1, 1), ("alleles", 2, 3), ("pad", 5, 3), ("next_len", 8, 8), ("codes", 16, 16)]
WIN_FIELDS = ["site", "allele", "len_a", "len_0", "site_order", "pad0", "pad1", "pad2"]


# ---- the half-key filters --------------------------------------------------------------------------------------------------------
def filter_hash(w0, w1):
    """hint_filter_hash (gtx_flat.hpp) on arrays of uint64 holding 32-bit values"""
    h = (w1 * np.uint64(0x9E3779B1)) & M32
    h ^= h >> np.uint64(15)
    h = (h + w0) & M32
    h = (h * np.uint64(0x85EBCA77)) & M32
    h ^= h >> np.uint64(16)
    h2 = (h * np.uint64(0x9E3779B1)) & M32
    return h, h2


def filter_slot(log2_words, w0, w1):
    """hint_filter_slot: (word, mask of up to four bits) of the half whose two planes are w0 / w1"""
    h, h2 = filter_hash(w0, w1)
    word = h >> np.uint64(32 - log2_words)
    one = np.uint64(1)
    mask = (one << (h2 >> np.uint64(27))) | (one << ((h2 >> np.uint64(22)) & np.uint64(31))) | (one << ((h2 >> np.uint64(17)) & np.uint64(31))) | \
           (one << ((h2 >> np.uint64(12)) & np.uint64(31)))
    return word, mask


def filter_present(filt, log2_words, w0, w1):
    word, mask = filter_slot(log2_words, w0, w1)
    return (filt[word].astype(np.uint64) & mask) == mask


def filter_log2_words(n_keys):
    """hint_filter_log2_words: 128 bits per key and side as a power of two of words, at least 2^7 and at most 2^28"""
    fl = 5
    while (1 << fl) < n_keys + 1 and fl < 28:
        fl += 1
    return min(fl + 2, 28)


def half_planes(half):
    """16 bases (2 bits each, the first in the top bits) of uint64 arrays -> the two planes the filter hashes: base j at bit j"""
    half = np.asarray(half, np.uint64)
    w0, w1 = np.zeros(half.shape, np.uint64), np.zeros(half.shape, np.uint64)
    for j in range(16):
        two = (half >> np.uint64(30 - 2 * j)) & np.uint64(3)
        w0 |= (two & np.uint64(1)) << np.uint64(j)
        w1 |= (two >> np.uint64(1)) << np.uint64(j)
    return w0, w1


def filters(keys, drop=None):
    """tables 3 and 4: the OR of every key's two halves' masks, and nothing else.  drop = (key index, side): that half is left out
    (what a build that forgets one looks like)"""
    keys = np.asarray(keys, np.uint64)
    fl = filter_log2_words(len(keys))
    out = []
    for side in range(2):
        f = np.zeros(1 << fl, np.uint64)
        half = (keys >> np.uint64(32)) if side == 0 else (keys & M32)
        w0, w1 = half_planes(half)
        word, mask = filter_slot(fl, w0, w1)
        if drop is not None and drop[1] == side:
            word, mask = np.delete(word, drop[0]), np.delete(mask, drop[0])
        np.bitwise_or.at(f, word.astype(np.int64), mask)
        out.append(f.astype(np.uint32))
    return out[0], out[1], fl


def _differing_bases(a, b):
    x = int(a) ^ int(b)
    return bin((x | (x >> 1)) & 0x5555555555555555).count("1")


class HintTablesRef:
    """tables(): the seven tables as uint32 words.  Everything else is kept for the fact tests of tests/hint_tables_cases.py."""

    def __init__(self, index, ograph, lgraph, is_sv_graph=False):
        keys, counts, labels = index
        self.keys = np.asarray(keys, np.uint64)
        assert np.all(self.keys[1:] > self.keys[:-1])
        self.counts = np.asarray(counts, np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.counts)])
        self.lab = np.asarray(labels, np.int64).reshape(-1, 3)
        self.sv = bool(is_sv_graph)
        g = self.g = {k: np.asarray(v).astype(np.int64) for k, v in ograph.items() if k in ("ref_order", "ref_len", "ref_nvar", "ref_first_var", "var_order", "var_len")}
        g["ref_dna"], g["var_dna"] = np.asarray(lgraph["ref_dna_off"], np.int64), np.asarray(lgraph["var_dna_off"], np.int64)
        self.dna = np.frombuffer(bytes(lgraph["dna"]), np.uint8)
        self.special = (np.asarray(ograph["ref_reach_poses"], np.int64), np.asarray(ograph["actual_poses"], np.int64))
        self.R = len(g["ref_order"])
        assert 0 < self.R and self.R - 1 < NO_SITE
        self.first = int(g["ref_order"][0])
        self.n = int(g["ref_order"][-1] + g["ref_len"][-1]) - self.first
        self._per_key()
        self._linear()
        self._windows()
        self._check_index_facts()

    def _check_index_facts(self):
        """What the arguments of tests/hint_tables_mutants/mutants.json take from the index, checked on every graph this class is made for:
        (1) one interval (start, end) lies under one set of sites -- every key with a label there has exactly those sites on it, or no site if
            there is none -- so a neighbour's label on a k-mer's own interval names one of the k-mer's own sites;
        (2) a label without a site on an interval belongs to one key only (the reference's bases there);
        (3) (asserted in tables(), per window position) a k-mer that reaches into its window's allele never has one label of allele 0 on a site."""
        vid = self.lab[:, 2]
        site = np.full(len(vid), -1, np.int64)
        g = self.g
        has = np.nonzero(g["ref_nvar"][:-1] > 0)[0]
        if len(has):
            at = np.searchsorted(g["ref_first_var"][has], np.where(vid == INVALID, 0, vid), side="right") - 1
            site = np.where(vid == INVALID, -1, has[np.maximum(at, 0)])
        key_of = np.repeat(np.arange(len(self.keys)), self.counts)
        under, plain = {}, {}
        for k, (s, e), r in zip(key_of.tolist(), self.lab[:, :2].tolist(), site.tolist()):
            under.setdefault((s, e), {}).setdefault(k, set()).add(r)
        for iv, per_key in under.items():
            sets = {frozenset(v) for v in per_key.values()}
            assert len(sets) == 1, "interval %s lies under %s" % (iv, sets)
            assert -1 not in next(iter(sets)) or len(per_key) == 1, "interval %s: a label without a site in %d keys" % (iv, len(per_key))

    # ---- a label's site and allele from its variant id
    def site_allele(self, vid):
        if vid == INVALID:
            return INVALID, 0
        g = self.g
        for r in np.nonzero((g["ref_first_var"][:-1] <= vid) & (vid < g["ref_first_var"][:-1] + g["ref_nvar"][:-1]) & (g["ref_nvar"][:-1] > 0))[0]:
            return int(r), int(vid - g["ref_first_var"][r])
        raise AssertionError("variant id %d lies on no site" % vid)

    def labels_of(self, k):
        """[(start, end, site, allele)] of key number k"""
        if k not in self._labels:
            self._labels[k] = [(int(s), int(e)) + self.site_allele(int(v)) for s, e, v in self.lab[self.off[k]:self.off[k + 1]]]
        return self._labels[k]

    def find(self, key):
        i = int(np.searchsorted(self.keys, np.uint64(key)))
        return i if i < len(self.keys) and int(self.keys[i]) == int(key) else -1

    # ---- per key: neighbours, half groups
    def _per_key(self):
        keys, nk = self.keys, len(self.keys)
        self._labels = {}
        # the 96 one-base variants, each looked up in the sorted keys
        self.nbr = np.full((nk, 96), -1, np.int64)
        for j in range(32):
            for d in (1, 2, 3):
                v = keys ^ (np.uint64(d) << np.uint64(2 * j))
                i = np.minimum(np.searchsorted(keys, v), max(nk - 1, 0))
                self.nbr[:, 3 * j + d - 1] = np.where(keys[i] == v, i, -1) if nk else -1
        self.nb = np.where(self.nbr >= 0, self.counts[np.maximum(self.nbr, 0)], 0).sum(1) if nk else np.zeros(0, np.int64)
        # keys that share the first / the last 16 bases
        self.group, self.gsize = [], []
        for half in (keys >> np.uint64(32), keys & M32):
            _, inv, cnt = np.unique(half, return_inverse=True, return_counts=True)
            members = {}
            for k, gi in enumerate(inv):
                members.setdefault(int(gi), []).append(k)
            self.group.append([members[int(gi)] for gi in inv])
            self.gsize.append(cnt[inv].astype(np.int64) if nk else np.zeros(0, np.int64))

    def neighbours(self, k):
        return [int(b) for b in self.nbr[k] if b >= 0]

    def nearest_sharer(self, k, side):
        """substitutions to the nearest OTHER key with key k's first (side 0) / last 16 bases; None: there is none"""
        others = [b for b in self.group[side][k] if b != k]
        return min(_differing_bases(self.keys[k], self.keys[b]) for b in others) if others else None

    def far_code(self, k, side):
        if self.gsize[side][k] > GROUP_LOOK_MAX:
            return 0  # (too crowded to look through)
        d = self.nearest_sharer(k, side)
        return 3 if d is None or d >= 8 else 2 if d >= 4 else 1 if d >= 3 else 0

    def _caps(self, k):
        return self.gsize[0][k] <= HE_CAP and self.gsize[1][k] <= HE_CAP and self.nb[k] <= NB_MAX

    def neighbours_same(self, k):
        """express4's seeding rule for an exact hit on key k whose labels are one interval on ONE site: every indexed Hamming-1 neighbour is that
        same interval on the same site (and the rule's wide form holds them: HINT_HE_CAP, HINT_NB_MAX)"""
        own = self.labels_of(k)
        if not self._caps(k) or len(own) > OWN_MAX or len({o[:3] for o in own}) != 1:
            return False
        if own[0][2] == INVALID:
            return self.nb[k] == 0  # (on no site: any neighbour is somebody else)
        return all(lb[:3] == own[0][:3] for b in self.neighbours(k) for lb in self.labels_of(b))

    def neighbours_known(self, k):
        """... over several sites: every neighbour label is the k-mer's own interval on one of its own sites"""
        own = self.labels_of(k)
        sites = {o[2] for o in own}
        if not self._caps(k) or INVALID in sites or len({o[:2] for o in own}) != 1:
            return False
        return all(lb[:2] == own[0][:2] and lb[2] in sites for b in self.neighbours(k) for lb in self.labels_of(b))

    def exact_verdict(self, k, start, end, site, allele):
        """a read k-mer equal to key k gets exactly the label (start, end, site, allele) and may be seeded from"""
        own = self.labels_of(k)
        if len(own) != 1 or own[0][:3] != (start, end, site) or (site != INVALID and own[0][3] != allele):
            return False
        return self.neighbours_same(k)

    # ---- the linear reference: bases, room, back, tail entries
    def _node_chars(self, off, n):
        return self.dna[off:off + n]

    def _linear(self):
        g, n, first = self.g, self.n, self.first
        self.chars = np.zeros(n, np.uint8)
        self.room, self.back = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.tail = np.zeros((n, 2), np.int64)
        for r in range(self.R):
            at, ln = int(g["ref_order"][r]) - first, int(g["ref_len"][r])
            self.chars[at:at + ln] = self._node_chars(int(g["ref_dna"][r]), ln)
            self.room[at:at + ln] = np.minimum(255, ln - np.arange(ln))
            self.back[at:at + ln] = np.minimum(255, np.arange(ln))
            if r + 1 == self.R:
                continue  # (the last node: no site behind it)
            fv, nv = int(g["ref_first_var"][r]), int(g["ref_nvar"][r])
            if nv:
                vat, vl = int(g["var_order"][fv]) - first, int(g["var_len"][fv])
                self.chars[vat:vat + vl] = self._node_chars(int(g["var_dna"][fv]), vl)
            if self.sv:
                continue
            x = TAIL_NODE
            alleles = [bytes(self._node_chars(int(g["var_dna"][fv + a]), int(g["var_len"][fv + a]))).decode("latin1") for a in range(nv)]
            if 2 <= nv <= 4 and all(len(a) == 1 and a in "ACGT" for a in alleles):
                x |= TAIL_OK | (nv << TAIL_NALL_SHIFT) | (min(255, int(g["ref_len"][r + 1])) << TAIL_NEXT_SHIFT)
                for a, s in enumerate(alleles):
                    x |= int(_NIBBLE[ord(s)]) << (TAIL_CODES_SHIFT + 4 * a)
            self.tail[at:at + ln] = (x, r)
        self.base = _NIBBLE[self.chars].astype(np.int64)

    # ---- the allele windows
    def site_order(self, r):
        return int(self.g["ref_order"][r] + self.g["ref_len"][r])

    def wants_windows(self, r):
        g = self.g
        if self.sv or r + 1 >= self.R:
            return False
        nv, fv = int(g["ref_nvar"][r]), int(g["ref_first_var"][r])
        lens = [int(x) for x in g["var_len"][fv:fv + nv]]
        if nv < 2 or nv > MASK_BITS or not 1 <= lens[0] <= WIN_ALLELE_MAX:
            return False
        if nv > 4 or any(x != 1 for x in lens):
            return True
        # a SNP: only with another site within a k-mer's reach (fewer than 31 reference bases between them)
        near_prev = r > 0 and g["ref_nvar"][r - 1] != 0 and g["ref_len"][r] < K - 1
        near_next = r + 2 < self.R and g["ref_nvar"][r + 1] != 0 and g["ref_len"][r + 1] < K - 1
        return bool(near_prev or near_next)

    def _windows(self):
        g = self.g
        self.win, self.site_win = [], np.zeros(self.R, np.int64)
        for r in range(self.R - 1):
            if not self.wants_windows(r):
                continue
            fv, first_w, count = int(g["ref_first_var"][r]), len(self.win), 0
            for a in range(1, int(g["ref_nvar"][r])):
                if 1 <= g["var_len"][fv + a] <= WIN_ALLELE_MAX and len(self.win) < WINDOWS_MAX:
                    self.win.append((r, a, int(g["var_len"][fv + a]), int(g["var_len"][fv]), self.site_order(r)))
                    count += 1
            self.site_win[r] = first_w | (count << 24) if count else 0
        self.win_base = (self.n // 64 + 5) * 64
        self.total = self.n if not self.win else self.win_base + len(self.win) * WIN_STRIDE + 256

    def win_order(self, w, local):
        """graph order of position `local` of window w: positions of an allele beyond the reference allele's last one are special positions"""
        site, allele, len_a, len_0, so = self.win[w]
        if local < WIN_BEFORE:
            return so - (WIN_BEFORE - local)
        k = local - WIN_BEFORE
        if k >= len_a:
            return so + len_0 + (k - len_a)
        pos, reach = so + k, so + len_0 - 1
        if pos <= reach:
            return pos
        hit = np.nonzero((self.special[0] == reach) & (self.special[1] == pos))[0]
        assert len(hit) == 1, "special position of site %d at %d: %s" % (site, pos, hit)
        return SPECIAL_START + int(hit[0])

    def window_source(self, w, local):
        """('allele', k) / ('linear', m) / None for position `local` of window w"""
        site, allele, len_a, len_0, so = self.win[w]
        if local < WIN_BEFORE:
            m = so - (WIN_BEFORE - local) - self.first
        elif local - WIN_BEFORE < len_a:
            return ("allele", local - WIN_BEFORE)
        elif local - WIN_BEFORE - len_a >= WIN_BEFORE:
            return None
        else:
            m = so + len_0 + (local - WIN_BEFORE - len_a) - self.first
        return ("linear", m) if 0 <= m < self.n else None

    # ---- the flags of one k-mer
    def flags_at(self, key, room, back, start, end, linear, near_free):
        """key: the 32 bases of the path from the position on in the index's 2-bit form (None: they are not 32 of A/C/G/T, or the path ends
        sooner); (start, end): where its label has to lie; near_free: the outcome of the 96 filter probes (kmers_and_probes())"""
        x, y, site = 0, room | (back << BACK_SHIFT), NO_SITE
        if key is None:
            return x | (site << SITE_SHIFT), y
        if near_free:
            y |= NEAR_FREE
        k = self.find(key)
        if k < 0:
            return x | (site << SITE_SHIFT), y
        y |= (self.far_code(k, 0) << FAR_LEFT_SHIFT) | (self.far_code(k, 1) << FAR_RIGHT_SHIFT)
        own = self.labels_of(k)
        here = all(o[:2] == (start, end) for o in own)
        sites = sorted({o[2] for o in own})
        if self.sv and any(o[2] != INVALID for o in own):
            return x | (site << SITE_SHIFT), y  # (no flags on variant labels of an SV graph)
        if here and len(own) == 1 and (own[0][2] == INVALID or own[0][3] == 0):
            o = own[0]
            site = NO_SITE if o[2] == INVALID else o[2]
            x |= SINGLE_OK | (L1 if self.gsize[0][k] == 1 else 0) | (R1 if self.gsize[1][k] == 1 else 0)
            if self.exact_verdict(k, start, end, o[2], 0):
                x |= EXACT_OK | (PAR if self.nb[k] else 0)
            if o[2] != INVALID and linear:
                xa, ya = self.snp_under(k, key, start, end, o[2])
                x, y = x | xa, y | ya
        elif here and 1 <= len(own) <= OWN_MAX and INVALID not in sites:
            if len(sites) == 1 and all(o[3] < MASK_BITS for o in own):
                # (one label names another allele than the reference's, or several alleles of a merged site spell the k-mer)
                if sites[0] < NO_SITE and self.neighbours_same(k):
                    site = sites[0]
                    x |= EXACT_OK | MULTI | (PAR if self.nb[k] else 0) | (sum({1 << o[3] for o in own}) << ALTIDX_SHIFT)
            elif len(sites) == 2 and sites[1] == sites[0] + 1 and all(o[3] < 4 for o in own) and len(own) >= 2:
                if sites[1] < NO_SITE and self.neighbours_known(k):
                    site = sites[0]
                    lo, hi = sum({1 << o[3] for o in own if o[2] == sites[0]}), sum({1 << o[3] for o in own if o[2] == sites[1]})
                    x |= EXACT_OK | TWO | (PAR if self.nb[k] else 0) | ((lo | (hi << 4)) << ALTIDX_SHIFT)
        return x | (site << SITE_SHIFT), y

    def snp_under(self, k, key, start, end, site):
        """HINT_ALT_OK and what goes with it: K lies over one site, a SNP, and every other allele's key passes the exact test with its own label"""
        g = self.g
        fv, nv = int(g["ref_first_var"][site]), int(g["ref_nvar"][site])
        off = int(g["var_order"][fv]) - start
        alleles = [bytes(self._node_chars(int(g["var_dna"][fv + a]), int(g["var_len"][fv + a]))).decode("latin1") for a in range(nv)]
        if not (2 <= nv <= 4 and 0 <= off < K and all(len(a) == 1 and a in "ACGT" for a in alleles)):
            return 0, 0
        shift = 2 * (K - 1 - off)
        idx_of, allele_keys = 0, [k]
        for a in range(1, nv):
            two = "ACGT".index(alleles[a])
            alt = (key & ~(3 << shift)) | (two << shift)
            ka = self.find(alt)
            if alt == key or (idx_of >> (2 * two)) & 3 or ka < 0 or not self.exact_verdict(ka, start, end, site, a):
                return 0, 0
            idx_of |= a << (2 * two)
            allele_keys.append(ka)
        near, other = (0, 1) if off < K // 2 else (1, 0)  # the half the SNP lies in / the other one
        alone = all(self.group[near][ka] == [ka] for ka in allele_keys) and sorted(self.group[other][k]) == sorted(allele_keys)
        refb = (key >> shift) & 3
        return ALT_OK | (idx_of << ALTIDX_SHIFT), (off << SNPOFF_SHIFT) | (SNP_GROUP if alone else 0) | (refb << REFB_SHIFT) | (nv << NV_SHIFT)

    # ---- everything
    @staticmethod
    def kmers_and_probes(base, filt):
        """per position of `base` (nibbles): whether the 32 bases from it on are all A/C/G/T, their key, and whether the filters hold NONE of the
        2 x 16 x 3 halves one substitution away from the key's halves"""
        f0, f1, fl = filt
        n = len(base) - K
        two = np.full(len(base), 255, np.uint64)
        for code, t in _TWO_OF.items():
            two[base == code] = t
        bad = np.concatenate([[0], np.cumsum(two == 255)])
        valid = (bad[K:] - bad[:-K])[:n] == 0
        key = np.zeros(n, np.uint64)
        for j in range(K):
            key = (key << np.uint64(2)) | np.where(valid, two[j:j + n], 0).astype(np.uint64)
        free = valid.copy()
        for side, f in ((0, f0), (1, f1)):
            w0, w1 = half_planes((key >> np.uint64(32)) if side == 0 else (key & M32))
            for j in range(16):
                for d in (1, 2, 3):
                    free &= ~filter_present(f, fl, w0 ^ (np.uint64(d & 1) << np.uint64(j)), w1 ^ (np.uint64(d >> 1) << np.uint64(j)))
        return valid, key, free

    def tables(self, filt=None):
        f0, f1, fl = filt or filters(self.keys)
        n, total = self.n, self.total
        base = np.zeros(total + K, np.int64)  # (nibbles of every table position; the padding holds none)
        room, back = np.zeros(total, np.int64), np.zeros(total, np.int64)
        tail = np.zeros((total, 2), np.int64)
        flags = np.zeros((total, 2), np.int64)
        base[:n], room[:n], back[:n], tail[:n] = self.base, self.room, self.back, self.tail
        for w, (site, allele, len_a, len_0, so) in enumerate(self.win):
            q0 = self.win_base + w * WIN_STRIDE
            fv = int(self.g["ref_first_var"][site])
            achars = self._node_chars(int(self.g["var_dna"][fv + allele]), len_a)
            for local in range(WIN_STRIDE):
                src = self.window_source(w, local)
                base[q0 + local] = 15  # (a window position without a base: N)
                if src is None:
                    continue
                if src[0] == "allele":
                    base[q0 + local] = _NIBBLE[achars[src[1]]]
                    continue
                m = src[1]
                base[q0 + local], room[q0 + local], back[q0 + local], tail[q0 + local] = self.base[m], self.room[m], self.back[m], self.tail[m]
                if tail[q0 + local][0] & TAIL_NODE and tail[q0 + local][1] == site:
                    tail[q0 + local][0] = TAIL_NODE  # (the window's own site: what lies there is the window's allele, not the reference's)
        valid, key, free = self.kmers_and_probes(base, (f0, f1, fl))
        for p in range(n):
            flags[p] = self.flags_at(int(key[p]) if valid[p] and p + K <= n else None, int(room[p]), int(back[p]), self.first + p, self.first + p + K - 1,
                                     True, free[p])
        for w, (site, allele, len_a, len_0, so) in enumerate(self.win):
            q0 = self.win_base + w * WIN_STRIDE
            for local in range(WIN_STRIDE):
                p = q0 + local
                none = (NO_SITE << SITE_SHIFT, int(room[p]) | (int(back[p]) << BACK_SHIFT))
                if local + K > WIN_STRIDE:
                    flags[p] = none
                elif local + K > WIN_BEFORE and local < WIN_BEFORE + len_a:  # the k-mer reaches into the allele: the window's path
                    # (checked fact (3), which index_build.hpp's SNP logic leans on: such a k-mer never has ONE label of allele 0 on a site)
                    kk = self.find(int(key[p])) if valid[p] else -1
                    own = self.labels_of(kk) if kk >= 0 else []
                    assert not (len(own) == 1 and own[0][2] != INVALID and own[0][3] == 0), "window %d position %d: %s" % (w, local, own)
                    flags[p] = self.flags_at(int(key[p]) if valid[p] else None, int(room[p]), int(back[p]), self.win_order(w, local) if valid[p] else 0,
                                             self.win_order(w, local + K - 1) if valid[p] else 0, False, free[p])
                else:
                    m = (so - (WIN_BEFORE - local) if local < WIN_BEFORE else so + len_0 + (local - WIN_BEFORE - len_a)) - self.first
                    flags[p] = flags[m] if 0 <= m < n else none
        planes = np.zeros(4 * (total // 32 + 8), np.uint32)
        for i in np.nonzero(base[:total])[0]:
            for b in range(4):
                if (int(base[i]) >> b) & 1:
                    planes[4 * (i >> 5) + b] |= np.uint32(1 << (i & 31))
        win = np.zeros((len(self.win), 8), np.uint32)
        for w, rec in enumerate(self.win):
            win[w, :5] = rec
        return [flags.astype(np.uint32).reshape(-1), planes, tail.astype(np.uint32).reshape(-1), f0, f1, win.reshape(-1),
                self.site_win.astype(np.uint32) if self.win else np.zeros(0, np.uint32)]


def describe(which, word_index, got, want):
    """the message of a differing word: table, position and field"""
    names = ["pos_flags", "planes", "tail_info", "filter side 0", "filter side 1", "windows", "site_win"]
    diff = int(got) ^ int(want)
    if which in (0, 2):
        p, half = divmod(word_index, 2)
        fields = (X_FIELDS if half == 0 else Y_FIELDS) if which == 0 else (TAIL_X_FIELDS if half == 0 else [("node", 0, 32)])
        bad = ["%s: %d, expected %d" % (nm, (int(got) >> lo) & ((1 << ln) - 1), (int(want) >> lo) & ((1 << ln) - 1))
               for nm, lo, ln in fields if (diff >> lo) & ((1 << ln) - 1)]
        return "table %d (%s) position %d word %s: %s" % (which, names[which], p, "xy"[half], "; ".join(bad))
    if which == 1:
        bits = [j for j in range(32) if (diff >> j) & 1]
        return "table 1 (planes) group %d plane %d: positions %s (0x%08x, expected 0x%08x)" % (word_index // 4, word_index % 4,
                                                                                                [32 * (word_index // 4) + j for j in bits[:8]], got, want)
    if which == 5:
        return "table 5 (windows) window %d field %s: %d, expected %d" % (word_index // 8, WIN_FIELDS[word_index % 8], got, want)
    if which == 6:
        return "table 6 (site_win) site %d: first %d count %d, expected first %d count %d" % (word_index, got & 0xFFFFFF, got >> 24, want & 0xFFFFFF, want >> 24)
    return "table %d (%s) word %d: 0x%08x, expected 0x%08x (bits 0x%08x)" % (which, names[which], word_index, got, want, diff)


def compare(got_tables, want_tables):
    """None when every word of every table is equal, else the message of the first difference of each table"""
    out = []
    for which, (got, want) in enumerate(zip(got_tables, want_tables)):
        got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
        if len(got) != len(want):
            out.append("table %d: %d words, expected %d" % (which, len(got), len(want)))
            continue
        d = np.nonzero(got != want)[0]
        if len(d):
            out.append(describe(which, int(d[0]), int(got[d[0]]), int(want[d[0]])) + " (%d words differ)" % len(d))
    return "\n".join(out) if out else None
