"""Frequency bands of the DCT spectrum: the partitions the band criterion scores with, and the host-side step that
turns a saved [C, K] spectrum into the reference's imp_*.npy score files. Needs no GPU.

imp_score(criterion="bands") (harness.py) writes band_score/<net>_limit<L>_<kind><K>/band_<stem>.npy: per hook point
the running mean of every channel's energy in each of K bands, [C, K] fp32. A band weighting - low-pass, high-pass,
anything - is chosen afterwards, here:

    python -m dct_pruning_amd.bands --spectrum band_score/resnet_50_limit5_square4 \\
        --band_weights 1,0.5,0.25,0 --out importance_score/resnet_50_lowpass

writes imp_<stem>.npy [C] fp32 = spectrum @ band_weights for every file (U2-Net-p: net.<module path>.npy, the
reference's own names), in the format prune_*.py --imp_score and
`python -m dct_pruning_amd.masks` read. All-ones weights reproduce the plain DCT energy (Parseval) up to rounding.
"""
import argparse
import os
import sys

import numpy as np

KINDS = ("square", "diag")
BAND_MAX = 8  # DCTS_BAND_MAX (include/dctscore.h)


def band_index(H, W, K, kind):
    """[H, W] int64: the band of every coefficient (u, v). Integer arithmetic throughout, so there is one answer.
    square: b = max(u*K // H, v*K // W) - L-infinity shells, band 0 holds DC;
    diag:   b = (u*W + v*H) * K // (2*H*W) - anti-diagonal stripes of the normalised frequency u/H + v/W."""
    if kind not in KINDS:
        raise ValueError("unknown band kind %r (expected one of %s)" % (kind, ", ".join(KINDS)))
    if H < 1 or W < 1 or not 1 <= K <= BAND_MAX:
        raise ValueError("partition needs H, W >= 1 and 1 <= K <= %d" % BAND_MAX)
    u = np.arange(H, dtype=np.int64)[:, None]
    v = np.arange(W, dtype=np.int64)[None, :]
    if kind == "square":
        return np.maximum(u * K // H, v * K // W)
    return (u * W + v * H) * K // (2 * H * W)


def partition(H, W, K, kind="square"):
    """One-hot [K, H, W] float32: weights[b, u, v] = 1 where coefficient (u, v) belongs to band b."""
    idx = band_index(H, W, K, kind)
    return (idx[None, :, :] == np.arange(K, dtype=np.int64)[:, None, None]).astype(np.float32)


def parse_band_weights(text):
    """'1,0.5,0.25,0' -> float64 vector."""
    try:
        w = np.array([float(t) for t in text.split(",")], dtype=np.float64)
    except ValueError:
        raise ValueError("band weights must be comma-separated numbers, got %r" % (text,))
    if w.size < 1:
        raise ValueError("no band weights given")
    return w


def apply_band_weights(spectrum, band_weights):
    """[C, K] spectrum -> [C] fp32 score: float64 product, rounded once."""
    spectrum = np.asarray(spectrum)
    w = np.asarray(band_weights, dtype=np.float64)
    if spectrum.ndim != 2 or w.ndim != 1 or spectrum.shape[1] != w.size:
        raise ValueError("a spectrum of shape %s does not take %d band weights" % (spectrum.shape, w.size))
    return np.ascontiguousarray((spectrum.astype(np.float64) @ w).astype(np.float32))


def score_file_name(band_file):
    """band_conv3.npy -> imp_conv3.npy; band_net.stage1.rebnconv1.relu_s1.npy -> net.stage1.rebnconv1.relu_s1.npy (the
    reference's U2-Net-p files carry no imp_ prefix)."""
    rest = band_file[len("band_"):]
    return rest if rest.startswith("net.") else "imp_" + rest


def collapse(spectrum_dir, band_weights, out_dir):
    """For every band_<stem>.npy [C, K] in spectrum_dir write out_dir/imp_<stem>.npy [C] fp32 = spectrum @ band_weights.
    Returns the list of files written (names only, sorted)."""
    names = sorted(f for f in os.listdir(spectrum_dir) if f.startswith("band_") and f.endswith(".npy"))
    if not names:
        raise ValueError("no band_*.npy files in %s" % spectrum_dir)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for f in names:
        spec = np.load(os.path.join(spectrum_dir, f), allow_pickle=False)
        if spec.ndim != 2:
            raise ValueError("%s holds shape %s, expected [C, K]" % (f, spec.shape))
        out = score_file_name(f)
        np.save(os.path.join(out_dir, out), apply_band_weights(spec, band_weights))
        written.append(out)
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description="Collapse a band spectrum directory into imp_*.npy score files")
    ap.add_argument("--spectrum", required=True, help="directory of band_*.npy files ([C, K] each)")
    ap.add_argument("--band_weights", required=True, help="one weight per band, e.g. 1,0.5,0.25,0")
    ap.add_argument("--out", required=True, help="directory for the imp_*.npy files")
    args = ap.parse_args(argv)
    try:
        weights = parse_band_weights(args.band_weights)
        written = collapse(args.spectrum, weights, args.out)
    except ValueError as exc:
        ap.error(str(exc))
    print("%d score files written to %s" % (len(written), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
