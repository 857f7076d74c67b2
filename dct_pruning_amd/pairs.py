"""Scores from pair matrices: the step between imp_score(criterion="gm", gm_pairs=True) and the mask tools.

A gm_<stem>.npy of that sweep holds D[c, k], the mean distance between the feature maps of channels c and k of a layer. The gm
criterion's own score is the row sum of D, and a sum cannot see what the criterion was built for: two exact duplicates that are
far from everything else get the same large sum, and both are kept. The rules here read the matrix instead. All run on the
host, in float64 on the file's values, and write one fp32 score per channel, high = keep, under the names prune_*.py
--imp_score and dct_pruning_amd.masks read:

    python -m dct_pruning_amd.pairs --matrix gm_score/vgg_16_bn_limit5_pairs --rule kcenter --out importance_score/vgg_kcenter

    sum      the row sum, rounded once: the gm criterion's score (up to the order of the summation);
    nn       the distance to the nearest OTHER channel, min_{k != c} D[c, k] (0 for a layer of one channel): a duplicate
             scores 0 however far the pair is from the rest. Both copies score 0, so a rate may still drop both;
    kcenter  farthest-point selection. The first channel is the one with the largest row sum; then, again and again, the
             channel whose distance to the nearest already selected one is largest. Every tie goes to the lowest index. The
             t-th selected channel (t = 0, 1, ...) scores C - t, so argsort(imp)[C - K:] is the first K selected for every K:
             the masks of all rates are nested, and of two duplicates the second is taken only after every channel that is
             not a copy of a selected one.
"""
import argparse
import os
import sys

import numpy as np

RULES = ("sum", "nn", "kcenter")


def _matrix(D):
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError("a pair matrix is square, got shape %s" % (D.shape,))
    return D.astype(np.float64)


def score_sum(D):
    return _matrix(D).sum(axis=1)


def score_nn(D):
    D = _matrix(D)
    C = D.shape[0]
    if C == 1:
        return np.zeros(1)
    off = D.copy()
    off[np.eye(C, dtype=bool)] = np.inf  # the channel itself is no neighbour
    return off.min(axis=1)


def kcenter_order(D):
    """The channels in the order farthest-point selection takes them (int64 [C])."""
    D = _matrix(D)
    C = D.shape[0]
    order = np.empty(C, dtype=np.int64)
    taken = np.zeros(C, dtype=bool)
    first = int(np.argmax(D.sum(axis=1)))  # argmax: the lowest index among equals
    order[0], taken[first] = first, True
    mind = D[:, first].copy()
    for t in range(1, C):
        nxt = int(np.argmax(np.where(taken, -np.inf, mind)))
        order[t], taken[nxt] = nxt, True
        mind = np.minimum(mind, D[:, nxt])
    return order


def score_kcenter(D):
    order = kcenter_order(D)
    C = order.size
    imp = np.empty(C)
    imp[order] = C - np.arange(C)
    return imp


_SCORE = {"sum": score_sum, "nn": score_nn, "kcenter": score_kcenter}


def score(D, rule):
    """[C, C] pair matrix -> [C] fp32 scores under `rule`: float64 arithmetic on the matrix's values, rounded once."""
    if rule not in _SCORE:
        raise ValueError("rule must be one of %s, got %r" % (", ".join(RULES), rule))
    return np.ascontiguousarray(_SCORE[rule](D).astype(np.float32))


def score_file_name(matrix_file):
    """gm_conv3.npy -> imp_conv3.npy; gm_net.stage1.rebnconv1.relu_s1.npy -> net.stage1.rebnconv1.relu_s1.npy (the rule of
    bands.score_file_name: the reference's U2-Net-p files carry no imp_ prefix)."""
    rest = matrix_file[len("gm_"):]
    return rest if rest.startswith("net.") else "imp_" + rest


def collapse(matrix_dir, rule, out_dir):
    """For every gm_<stem>.npy [C, C] in matrix_dir write out_dir/imp_<stem>.npy [C] fp32 = score(matrix, rule). Returns the
    list of files written (names only, sorted)."""
    if rule not in _SCORE:
        raise ValueError("rule must be one of %s, got %r" % (", ".join(RULES), rule))
    names = sorted(f for f in os.listdir(matrix_dir) if f.startswith("gm_") and f.endswith(".npy"))
    if not names:
        raise ValueError("no gm_*.npy files in %s" % matrix_dir)
    mats = []
    for f in names:  # every file is checked before the first one is written
        D = np.load(os.path.join(matrix_dir, f), allow_pickle=False)
        if D.ndim != 2 or D.shape[0] != D.shape[1]:
            raise ValueError("%s holds shape %s, expected a square [C, C] pair matrix (a sweep with gm_pairs)" % (f, D.shape))
        mats.append(D)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for f, D in zip(names, mats):
        out = score_file_name(f)
        np.save(os.path.join(out_dir, out), score(D, rule))
        written.append(out)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description="Turn a directory of [C, C] pair matrices into imp_*.npy score files")
    ap.add_argument("--matrix", required=True, help="directory of gm_*.npy files ([C, C] each; imp_score(..., gm_pairs=True))")
    ap.add_argument("--rule", required=True, choices=RULES,
                    help="sum: row sum (the gm score); nn: distance to the nearest other channel; kcenter: farthest-point order")
    ap.add_argument("--out", required=True, help="directory for the imp_*.npy files")
    args = ap.parse_args(argv)
    try:
        written = collapse(args.matrix, args.rule, args.out)
    except ValueError as exc:
        ap.error(str(exc))
    print("%d score files written to %s" % (len(written), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
