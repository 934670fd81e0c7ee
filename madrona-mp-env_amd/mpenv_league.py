"""League bookkeeping on the host from the device's standings table
(include/mpenv_league.h, DESIGN.md §2 definition 20).  numpy only.

The table is int64 [P+1, P+1, 8]: cell [i, j] holds what the episodes between
team 0 of bucket i and team 1 of bucket j added -- episodes, wins of team 0,
wins of team 1, draws, kills of team 0 / 1, zone points of team 0 / 1.
Bucket P is everything that is no league policy (external, out of range,
mixed)."""
import numpy as np

EPISODES, WINS0, WINS1, DRAWS, KILLS0, KILLS1, ZONE0, ZONE1 = range(8)
MAX_WEIGHT = 65535


def win_rates(table):
    """Team 0's view: [P+1, P+1] float64, (wins of team 0 + draws / 2) / decided episodes of the
    cell, where decided = wins 0 + wins 1 + draws; NaN for a cell without a decided episode."""
    t = np.asarray(table, np.int64)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 8:
        raise ValueError("table must be [P+1, P+1, 8]")
    decided = (t[..., WINS0] + t[..., WINS1] + t[..., DRAWS]).astype(np.float64)
    score = t[..., WINS0] + 0.5 * t[..., DRAWS]
    return np.divide(score, decided, out=np.full(decided.shape, np.nan), where=decided > 0)


def symmetric_win_rates(table):
    """[P+1, P+1]: how row i fares against column j over both seatings, (i as team 0 against j) and
    (j as team 0 against i) pooled; NaN where the pair has no decided episode."""
    t = np.asarray(table, np.int64)
    wins = t[..., WINS0] + t[..., WINS1].T
    draws = t[..., DRAWS] + t[..., DRAWS].T
    decided = (wins + wins.T + draws).astype(np.float64)
    return np.divide(wins + 0.5 * draws, decided, out=np.full(decided.shape, np.nan), where=decided > 0)


def pfsp_weights(table, home=None, power=1.0, scale=MAX_WEIGHT):
    """Integer prioritised-fictitious-self-play weights [P+1, P] for MPENV_LEAGUE_WEIGHTS: row i
    weighs opponent j by (1 - winrate(i against j)) ** power, with win rates pooled over both
    seatings and 0.5 for a pair that has not met; each row is scaled so that its largest entry is
    `scale` (at most 65535, what the kernel reads) and rounded; an opponent with a positive
    priority keeps weight >= 1.  A row whose priorities are all zero (i beats everyone every time)
    is uniform.  home: the rows to compute (an index or a list); the others are all 1.  None: all."""
    t = np.asarray(table, np.int64)
    P = t.shape[0] - 1
    if not 1 <= scale <= MAX_WEIGHT:
        raise ValueError("scale must be in [1, 65535]")
    wr = symmetric_win_rates(t)[:, :P]
    wr = np.where(np.isnan(wr), 0.5, wr)
    pri = (1.0 - wr) ** float(power)
    out = np.ones((P + 1, P), np.int32)
    rows = range(P + 1) if home is None else np.atleast_1d(home)
    for i in rows:
        top = pri[i].max()
        if top <= 0:
            out[i] = scale
            continue
        w = np.rint(pri[i] / top * scale).astype(np.int64)
        out[i] = np.where(pri[i] > 0, np.maximum(w, 1), 0)
    return out
