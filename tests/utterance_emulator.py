"""Numpy / plain-Python restatement of whole-utterance encoding (include/aewavenet.h: aew_utt_row_t, AEW_OP_MEL_TILE,
AEW_OP_CODE_STITCH; ae_wavenet_amd/codes.py: tile_plan): the work list as loops over utterances and windows, the two
ops element by element, the record checks of the launchers, and the hand-cut windows the product is compared with.
Written from the header's text; shares no code with the package."""
import numpy as np

ROW = np.dtype([("src", "<i8"), ("dst", "<i8"), ("pitch", "<i4"), ("avail", "<i4"), ("n_valid", "<i4"), ("pad_", "<i4")])


def n_codes(F, s, rf):
    return 0 if F < rf else (F - rf) // s + 1


def case_frames(E, s, rf):
    """The ten frame counts of the issue, in its order: 0 codes; 1 code; one frame more (still 1 code for s = 2); 2
    codes; one frame short of a full window; a full window; one frame more; a second window holding one code; exactly
    three windows; three windows plus E - 1 codes."""
    mel_len = s * (E - 1) + rf
    return [rf - 1, rf, rf + 1, rf + s, mel_len - 1, mel_len, mel_len + 1, mel_len + s,
            rf + s * (3 * E - 1), rf + s * (4 * E - 2)]


MIX = (8, 0, 3, 9, 5, 1, 7, 4, 6, 2)


def mixed_frames(E, s, rf):
    """The ten cases mixed into one call, the long ones between the short ones, and one more utterance of rf frames
    behind them: the ten alone make 15 windows, a whole number of batches at B = 3 - with the extra one the last batch
    has two idle rows."""
    cases = case_frames(E, s, rf)
    return [cases[i] for i in MIX] + [rf]


def tile_plan(frames, E, s, rf, B):
    """(offsets [U + 1], rows): rows = one dict per batch row - utt (-1 idle), window, start, avail, n_valid, dst -
    padded with idle rows to a multiple of B."""
    mel_len = s * (E - 1) + rf
    offsets, rows = [0], []
    for u, F in enumerate(frames):
        N = n_codes(F, s, rf)
        w = 0
        while w * E < N:
            start = w * s * E
            rows.append(dict(utt=u, window=w, start=start, avail=min(mel_len, F - start), n_valid=min(E, N - w * E),
                             dst=offsets[-1] + w * E))
            w += 1
        offsets.append(offsets[-1] + N)
    n_rows = len(rows)
    while len(rows) % B:
        rows.append(dict(utt=-1, window=0, start=0, avail=0, n_valid=0, dst=0))
    return offsets, rows, n_rows


def bases_of(frames, n_mel):
    out, at = [], 0
    for F in frames:
        out.append(at)
        at += n_mel * F
    return out, at


def table(rows, frames, bases):
    rec = np.zeros(len(rows), ROW)
    for k, r in enumerate(rows):
        if r["utt"] >= 0:
            rec[k] = (bases[r["utt"]] + r["start"], r["dst"], frames[r["utt"]], r["avail"], r["n_valid"], 0)
    return rec


def tile_ok(r, n_mel, mel_len, n_src):
    a = int(r["avail"])
    if a < 0 or a > mel_len:
        return False
    if a == 0:
        return True
    last = int(r["src"]) + (n_mel - 1) * int(r["pitch"]) + a - 1
    return int(r["src"]) >= 0 and int(r["pitch"]) >= a and last < n_src


def stitch_ok(r, E, n_dst):
    n = int(r["n_valid"])
    if n < 0 or n > E:
        return False
    return n == 0 or (int(r["dst"]) >= 0 and int(r["dst"]) + n <= n_dst)


def locate(r, n_mel, mel_len, E, n_src, n_dst, i):
    """(src or -1, avail, n_valid) of flat element i of the row's in_mel, None where the record is refused."""
    if not (tile_ok(r, n_mel, mel_len, n_src) and stitch_ok(r, E, n_dst)) or not 0 <= i < n_mel * mel_len:
        return None
    c, t = divmod(i, mel_len)
    return (int(r["src"]) + c * int(r["pitch"]) + t if t < r["avail"] else -1), int(r["avail"]), int(r["n_valid"])


def mel_tile(tbl, first, B, mel, n_mel, mel_len):
    """in_mel (B, n_mel, mel_len) float32; the copied elements keep their bits, the rest are +0.0."""
    out = np.zeros((B, n_mel, mel_len), np.float32)
    for b in range(B):
        r = tbl[first + b]
        for c in range(n_mel):
            a = int(r["avail"])
            at = int(r["src"]) + c * int(r["pitch"])
            out[b, c, :a] = mel[at:at + a]
    return out


def code_stitch(tbl, first, B, ind, min_dist, codes, dist, E):
    """In place on codes (int64) and - unless None - dist (float32); ind / min_dist (B * E,)."""
    for b in range(B):
        r = tbl[first + b]
        n, d = int(r["n_valid"]), int(r["dst"])
        codes[d:d + n] = ind[b * E:b * E + n]
        if dist is not None:
            dist[d:d + n] = min_dist[b * E:b * E + n]


def cut_windows(mel, E, s, rf):
    """mel (n_mel, F) -> (windows (W, n_mel, mel_len) cut by hand at hop s * E and zero-padded, [codes kept per window])."""
    n_mel, F = mel.shape
    mel_len, N = s * (E - 1) + rf, n_codes(F, s, rf)
    wins, keep = [], []
    for w in range(-(-N // E)):
        x = np.zeros((n_mel, mel_len), np.float32)
        part = mel[:, w * s * E:w * s * E + mel_len]
        x[:, :part.shape[1]] = part
        wins.append(x)
        keep.append(min(E, N - w * E))
    return (np.stack(wins) if wins else np.zeros((0, n_mel, mel_len), np.float32)), keep
