"""Matching the reads of ended plate tracks against a watchlist, on the CPU: ``watch_match_np`` is the written-down
specification of ``lp_watch_match`` (include/lp_hip.h, csrc/lp_watch.hip), which matches it on every int32, and the CPU path of
``Inferer(track=True, watchlist=...)``.  All arithmetic is integer except one fp32 product per position; every reduction (the
minimum of a key, an integer count) is independent of its order, so the result is reproducible bit for bit by construction.

The reference has nothing here: its Inferer treats frames independently (yolov6/core/inferer.py).

A voted read is wrong in one position often enough (8/B, 0/D/Q, 2/Z, 5/S) that a useful lookup tolerates a misread and charges
less for a position the vote itself was unsure about.  The read is positional -- eight heads, one per character -- so the measure
is a weighted Hamming distance, not an edit distance.

Rules:
  watchlist: ``entries`` uint8 [N, 8], 0 <= N <= MAX_ENTRIES (2^24), one row per plate, one id per head.  Ids 0..63 are class
     ids, 255 is the wildcard ``WILD`` (the position is not compared), ids 64..254 match nothing (``check_entries`` refuses them;
     the kernel and this function still define them: a mismatch of weight 16);
  confusion table: ``confuse`` uint8 [3, 64, 64] with values 0..16, in sixteenths; group 0 is head 0 (province), group 1 head 1
     (alphabet), group 2 heads 2..7; the row is the read id, the column the entry id; None = 16 everywhere.  The diagonal is
     never read;
  reads: per stream s the lines j < min(max(ended_count[s], 0), max_ended) of ``ended_i`` / ``ended_f`` as ``PlateTracker.update``
     leaves them: best[p] = ended_i[s, j, 4 + p], share[p] = ended_f[s, j, p];
  per position p of entry e, w = entries[e, p]:
     q_p = min((int)(share[p] * 255.0f), 255) + 1 if share[p] > 0 (the fp32 product, truncated; false for NaN), else 1: 1..256;
     w == WILD: cost 0, no mismatch;  0 <= best[p] < 64 and w == best[p]: cost 0, no mismatch;
     otherwise one mismatch of cost q_p * c, c = confuse[g(p)][best[p]][w] when best[p] and w are both in 0..63, else 16;
  mism(e), cost(e): the int32 sums over the eight positions, cost <= 8 * 256 * 16 = 32768 = MAX_COST;
  entry e is accepted iff mism(e) <= max_mismatch (0..8) and cost(e) <= max_cost (0..32768);
  match_i int32 [S, max_ended, 4], line-parallel to ended_i: (entry, mismatches, cost, n_hits) -- the accepted entry with the
     smallest (cost, index) and the number of accepted entries (above 1: the match is ambiguous; duplicates count, the lowest
     index wins); (-1, 0, 0, 0) for a line without an accepted entry, for every line at or past the stream's count, and for
     every line when N = 0.

One lost or gained character (``indel=1``; ``lp_watch_match_indel``).  When two narrow glyphs merge, a rivet is read as a
character, or a 7-character plate is read as 8, every later head moves by one and the positional measure charges four or five
mismatches for one error.  Heads 2..7 share one alphabet and one confusion group, so read head p may be compared with entry head
p + 1 or p - 1 by the same rule.  Rules 1-3 above give, per read, position p and entry byte w, a pair (cost, mismatch); call it
U[p] for w = entries[e, p], L[p] (p in 2..6) for w = entries[e, p + 1] and R[p] (p in 3..7) for w = entries[e, p - 1].  WILD, ids
64..254 and a best[p] outside 0..63 behave in L and R as they do in U.  An entry is scored under 12 alignments, each
U[0] + U[1] plus:
  code 0, unshifted: sum U[2..7];
  codes 1..5, the read lost the character at entry head k = 2..6 (code k - 1): sum U[2..k-1] + sum L[k..6]; read head 7 is not
     compared;
  codes 6..10, the read gained a character at read head k = 2..6 (code k + 4): sum U[2..k-1] + sum R[k+1..7]; read head k and
     entry head 7 are not compared;
  code 11, the error is at the end: sum U[2..6]; head 7 is compared on neither side.
Codes 1..11 add ``gap_cost`` (cost units, 0..COST_SCALE, default COST_SCALE: one fully confident mismatch) to the cost and 1 to
the mismatches, so a shifted alignment compares at most seven positions plus the gap and its cost stays <= MAX_COST.  The
entry's score is the alignment with the smallest (cost, mismatches, code); the entry is accepted iff THAT alignment has
mismatches <= max_mismatch and cost <= max_cost.  Across entries nothing changes: the smallest (cost, index) wins, n_hits counts
the accepted entries.  match_i's mismatches count the gap; match_align int32 [S, max_ended] is the winning entry's code, 0 on a
line without a hit.  With ``indel=0`` only code 0 exists and the result is the positional one on every int32.  With the default
max_mismatch = 1 a shifted read must be otherwise exact.  ``align_text`` names a code: ``-``, ``del@k``, ``ins@k``, ``end``.

What it does not do: at most ONE insertion or deletion, and only in heads 2..7 (heads 0 and 1 have other alphabets; a read that
lost or gained two characters matches nothing nearby; without ``indel`` none at all); the sightings log stays positional
(``yolov6.utils.sight``); no alert while a track is still live (ended records only: ``yolov6.utils.watch_live`` does that); one
best entry plus a count, not a ranked list; no persistence or update in place of the list (a changed list is a new
``Watchlist``).
"""
import numpy as np

from yolov6.utils.track import ENDED_COLS, HEADS, MAX_CLS

WILD = 255
MAX_ENTRIES = 1 << 24
MAX_COST = 8 * 256 * 16       # 32768
FULL = 16                     # the weight of an unlisted confusion, in sixteenths
COST_SCALE = 256 * FULL       # cost units of one fully confident, unlisted mismatch
GROUP_OF = (0, 1, 2, 2, 2, 2, 2, 2)
N_ALIGN = 12                  # alignment codes of ``indel=1``: 0 unshifted, 1..5 del@2..6, 6..10 ins@2..6, 11 end
f32 = np.float32


def check_entries(entries):
    """``entries`` as the uint8 [N, 8] array of a watchlist (ValueError: shape, N above 2^24, an id in 64..254)."""
    a = np.asarray(entries)
    if a.size == 0:
        return np.zeros((0, HEADS), np.uint8)
    if a.ndim != 2 or a.shape[1] != HEADS:
        raise ValueError('entries must be [N, %d]' % HEADS)
    if a.dtype.kind not in 'iu':
        raise ValueError('entries must be integers')
    if len(a) > MAX_ENTRIES:
        raise ValueError('a watchlist holds at most %d entries' % MAX_ENTRIES)
    bad = np.nonzero(~(((a >= 0) & (a < MAX_CLS)) | (a == WILD)))
    if len(bad[0]):
        raise ValueError('entry %d, position %d: id %d (need 0..%d, or %d for the wildcard)'
                         % (bad[0][0], bad[1][0], a[bad[0][0], bad[1][0]], MAX_CLS - 1, WILD))
    return np.ascontiguousarray(a, dtype=np.uint8)


def check_confuse(confuse):
    """``confuse`` as the uint8 [3, 64, 64] table (None: all 16); ValueError for another shape or a value above 16."""
    if confuse is None:
        return np.full((3, MAX_CLS, MAX_CLS), FULL, np.uint8)
    c = np.asarray(confuse)
    if c.shape != (3, MAX_CLS, MAX_CLS) or c.dtype.kind not in 'iu':
        raise ValueError('confuse must be integers [3, %d, %d]' % (MAX_CLS, MAX_CLS))
    if c.min() < 0 or c.max() > FULL:
        raise ValueError('confuse holds sixteenths: 0..%d' % FULL)
    return np.ascontiguousarray(c, dtype=np.uint8)


class WatchlistNp:
    """A checked watchlist on the host: what ``PlateTrackerNp.enable_watch`` takes (``runtime.Watchlist`` is the device form)."""

    def __init__(self, entries, confuse=None, device=None):
        self.entries_np = check_entries(entries)
        self.confuse_np = None if confuse is None else check_confuse(confuse)
        self.n = len(self.entries_np)
        self.last_align = None

    def match(self, ended_i, ended_f, ended_count, max_mismatch=1, max_cost=None, indel=0, gap_cost=None):
        """``watch_match_np`` on this list; ``max_cost`` a float in fully confident mismatches (``cost_units``; None: no limit).
        ``indel=1`` tolerates one lost or gained character at ``gap_cost`` fully confident mismatches (``gap_units``; None: 1) and
        leaves match_align [S, max_ended] int32 in ``last_align`` (None without it)."""
        self.last_align = None
        if not check_indel(indel, gap_units(gap_cost))[0]:
            return watch_match_np(self.entries_np, self.confuse_np, ended_i, ended_f, ended_count, max_mismatch, cost_units(max_cost))
        m, self.last_align = watch_match_np(self.entries_np, self.confuse_np, ended_i, ended_f, ended_count, max_mismatch,
                                            cost_units(max_cost), 1, gap_units(gap_cost), align=True)
        return m


def cost_units(x):
    """``max_cost`` given in fully confident mismatches (a float; None: no limit) as the integer of the rule:
    clamp(floor(x * 4096 + 0.5), 0, 32768)."""
    if x is None:
        return MAX_COST
    x = float(x)
    if x != x:
        raise ValueError('max_cost is NaN')
    return int(min(max(np.floor(x * COST_SCALE + 0.5), 0), MAX_COST))


def check_params(max_mismatch, max_cost):
    """(max_mismatch, max_cost) as the integers of the rule (ValueError outside 0..8 / 0..32768)."""
    mm, mc = int(max_mismatch), int(max_cost)
    if mm != max_mismatch or not 0 <= mm <= HEADS:
        raise ValueError('max_mismatch must be an integer in 0..%d' % HEADS)
    if mc != max_cost or not 0 <= mc <= MAX_COST:
        raise ValueError('max_cost must be an integer in 0..%d (cost_units converts a float)' % MAX_COST)
    return mm, mc


def gap_units(x):
    """``gap_cost`` given in fully confident mismatches (a float; None: 1) as the integer of the rule:
    clamp(floor(x * 4096 + 0.5), 0, 4096)."""
    if x is None:
        return COST_SCALE
    x = float(x)
    if x != x:
        raise ValueError('gap_cost is NaN')
    return int(min(max(np.floor(x * COST_SCALE + 0.5), 0), COST_SCALE))


def check_indel(indel, gap_cost):
    """(indel, gap_cost) as the integers of the rule (ValueError outside 0..1 / 0..4096)."""
    i, g = int(indel), int(gap_cost)
    if i != indel or i not in (0, 1):
        raise ValueError('indel must be 0 or 1')
    if g != gap_cost or not 0 <= g <= COST_SCALE:
        raise ValueError('gap_cost must be an integer in 0..%d (gap_units converts a float)' % COST_SCALE)
    return i, g


def align_text(code):
    """An alignment code as the tools print it: ``-`` (0), ``del@k`` (1..5, k = 2..6: the entry's head k is missing from the read),
    ``ins@k`` (6..10, k = 2..6: the read's head k is not in the entry), ``end`` (11)."""
    code = int(code)
    if not 0 <= code < N_ALIGN:
        raise ValueError('alignment code %d outside 0..%d' % (code, N_ALIGN - 1))
    return '-' if code == 0 else 'del@%d' % (code + 1) if code <= 5 else 'ins@%d' % (code - 4) if code <= 10 else 'end'


def confuse_table(pairs, group=2, weight=4, names=None):
    """A symmetric confusion table: 16 everywhere, ``weight`` (sixteenths, 0..16) at [group][a][b] and [group][b][a] for every
    pair (a, b) of ``pairs``: ids, or characters looked up in ``names`` (the group's name list of the data yaml).  A two-character
    string is a pair, so ``'0D 0Q 8B'.split()`` is a list of pairs."""
    weight = int(weight)
    if not 0 <= int(group) <= 2 or not 0 <= weight <= FULL:
        raise ValueError('confuse_table needs group in 0..2 and weight in 0..%d' % FULL)
    table = check_confuse(None)

    def ident(v):
        if isinstance(v, (int, np.integer)):
            i = int(v)
        else:
            if names is None or str(v) not in [str(n) for n in names]:
                raise ValueError('confusable %r is not among the names' % (v,))
            i = [str(n) for n in names].index(str(v))
        if not 0 <= i < MAX_CLS:
            raise ValueError('confusable id %d outside 0..%d' % (i, MAX_CLS - 1))
        return i

    for pair in pairs:
        if len(pair) != 2:
            raise ValueError('confusable %r is not a pair' % (pair,))
        a, b = ident(pair[0]), ident(pair[1])
        table[group, a, b] = table[group, b, a] = weight
    return table


def parse_watchlist(lines, pro_names=None, alp_names=None, ads_names=None):
    """uint8 [N, 8] of a watchlist file's lines, one plate per line: eight space-separated ids with ``*`` for the wildcard, or
    the plate text, one character per head looked up in the three name lists of the data yaml with ``*`` / ``?`` as wildcard:
    the inverse of ``track.plate_text``.  Blank lines and ``#`` comments are skipped; a bad line raises ValueError naming it."""
    lists = None
    if pro_names and alp_names and ads_names:
        lists = [[str(n) for n in names] for names in [pro_names, alp_names] + [ads_names] * 6]
    out = []
    for no, line in enumerate(lines, 1):
        text = line.split('#', 1)[0].strip()
        if not text:
            continue
        tok = text.split()
        try:
            if len(tok) == HEADS:
                row = [WILD if t == '*' else int(t) for t in tok]
                if not all(0 <= v < MAX_CLS or v == WILD for v in row):
                    raise ValueError('ids must be 0..%d or *' % (MAX_CLS - 1))
            elif len(tok) == 1 and lists is not None:
                row = _text_ids(tok[0], lists)
            else:
                raise ValueError('need eight ids' + (' or a plate text' if lists is not None else ' (plate text needs the name lists)'))
        except ValueError as e:
            raise ValueError('watchlist line %d (%r): %s' % (no, text, e)) from None
        out.append(row)
    return check_entries(np.array(out, np.uint8).reshape(-1, HEADS))


def entry_text(ids, pro_names=None, alp_names=None, ads_names=None):
    """An entry as ``parse_watchlist`` reads it back: ``track.plate_text`` with ``*`` for the wildcard (the ids, space-separated,
    without names or for an id outside its list)."""
    ids = [int(v) for v in ids]
    if len(ids) != HEADS:
        raise ValueError('entry_text needs eight ids')
    if pro_names and alp_names and ads_names:
        lists = [pro_names, alp_names] + [ads_names] * 6
        if all(i == WILD or 0 <= i < len(names) for i, names in zip(ids, lists)):
            return ''.join('*' if i == WILD else str(names[i]) for i, names in zip(ids, lists))
    return ' '.join('*' if i == WILD else str(i) for i in ids)


def confusable_pairs(spec):
    """The pairs of a ``--watch-confusable`` value: a string of space-separated tokens or a list of them; a token is two characters
    (``0D``) or two ids joined by a colon (``0:13``)."""
    out = []
    for tok in (spec.split() if isinstance(spec, str) else list(spec or ())):
        if isinstance(tok, str) and ':' in tok:
            a, b = tok.split(':', 1)
            tok = (int(a), int(b))
        out.append(tok)
    return out


def _text_ids(text, lists):
    """The eight ids of a plate text: per head the longest name that the rest of the text starts with."""
    row, at = [], 0
    for names in lists:
        if at < len(text) and text[at] in '*?':
            row.append(WILD)
            at += 1
            continue
        hit = max((n for n in names if n and text.startswith(n, at)), key=len, default=None)
        if hit is None:
            raise ValueError('no name of head %d at %r' % (len(row), text[at:]))
        i = names.index(hit)
        if i >= MAX_CLS:
            raise ValueError('id %d of head %d is above %d' % (i, len(row), MAX_CLS - 1))
        row.append(i)
        at += len(hit)
    if at != len(text):
        raise ValueError('%r is left over after eight characters' % text[at:])
    return row


def position_weight(share):
    """q_p int32 of fp32 vote shares: min((int)(share * 255.0f), 255) + 1 where share > 0 (false for NaN), else 1."""
    share = np.asarray(share, f32)
    with np.errstate(all='ignore'):
        t = np.minimum(share * f32(255.0), f32(255.0))         # the clamp before the conversion: +inf and 2.0 give 255
        pos = share > 0
        return np.where(pos, np.where(pos, t, f32(0)).astype(np.int32) + 1, 1).astype(np.int32)


def watch_match_np(entries, confuse, ended_i, ended_f, ended_count, max_mismatch, max_cost, indel=0, gap_cost=COST_SCALE, align=False):
    """match_i int32 [S, max_ended, 4] of the module's rule, or (match_i, match_align int32 [S, max_ended]) with ``align=True``.
    Per read and position one table over the 256 byte values of an entry id gives (cost, mismatch); an entry's totals are eight
    gathers (eighteen with ``indel=1``), so N = 10^5 with a few dozen reads takes well under a second.  Unlike
    ``check_entries`` this takes ids 64..254, as the kernel must."""
    entries = np.ascontiguousarray(entries, dtype=np.uint8).reshape(-1, HEADS)
    confuse = check_confuse(confuse)
    mm, mc = check_params(max_mismatch, max_cost)
    indel, gap = check_indel(indel, gap_cost)
    ended_i, ended_f = np.asarray(ended_i, np.int32), np.asarray(ended_f, f32)
    ended_count = np.asarray(ended_count).astype(np.int64).reshape(-1)
    S, max_ended = ended_i.shape[:2]
    if ended_i.shape != (S, max_ended, ENDED_COLS) or ended_f.shape != ended_i.shape or len(ended_count) != S:
        raise ValueError('ended_i / ended_f must be [S, max_ended, %d] and ended_count [S]' % ENDED_COLS)
    out = np.zeros((S, max_ended, 4), np.int32)
    out[:, :, 0] = -1
    out_a = np.zeros((S, max_ended), np.int32)
    N = len(entries)
    ids = np.arange(256)
    for s in range(S if N else 0):
        for j in range(min(max(int(ended_count[s]), 0), max_ended)):
            best, q = ended_i[s, j, 4:12], position_weight(ended_f[s, j, :HEADS])
            tab = []                                                        # per position: (cost, mismatch) of every entry byte
            for p in range(HEADS):
                b = int(best[p])
                c = np.full(256, FULL, np.int32)
                miss = ids != WILD
                if 0 <= b < MAX_CLS:
                    c[:MAX_CLS] = confuse[GROUP_OF[p], b]
                    miss &= ids != b
                tab.append((np.where(miss, int(q[p]) * c, 0).astype(np.int32), miss.astype(np.int32)))

            def pair(p, col):                                               # read head p against entry head col, as one word
                w = entries[:, col]
                return (tab[p][0][w].astype(np.int64) << 8) | tab[p][1][w]

            U = [pair(p, p) for p in range(HEADS)]
            word = [sum(U)]                                                 # code 0; cost << 8 | mismatches, mismatches <= 8
            if indel:
                L = {p: pair(p, p + 1) for p in range(2, 7)}
                R = {p: pair(p, p - 1) for p in range(3, 8)}
                gapw = (gap << 8) | 1
                for k in range(2, 7):                                       # codes 1..5
                    word.append(U[0] + U[1] + sum(U[2:k]) + sum(L[p] for p in range(k, 7)) + gapw)
                for k in range(2, 7):                                       # codes 6..10
                    word.append(U[0] + U[1] + sum(U[2:k]) + sum(R[p] for p in range(k + 1, 8)) + gapw)
                word.append(U[0] + U[1] + sum(U[2:7]) + gapw)               # code 11
            word = np.stack(word)
            code = np.argmin(word, axis=0)                                  # the first (lowest) code of the smallest (cost, mismatches)
            win = word[code, np.arange(N)]
            cost, mism = (win >> 8).astype(np.int32), (win & 255).astype(np.int32)
            ok = (mism <= mm) & (cost <= mc)
            n = int(ok.sum())
            if n:
                e = int(np.argmin(np.where(ok, cost, MAX_COST + 1)))        # the first index of the smallest accepted cost
                out[s, j] = (e, mism[e], cost[e], n)
                out_a[s, j] = code[e]
    return (out, out_a) if align else out
