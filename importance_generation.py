#!/usr/bin/env python3
"""Importance Assessment — drop-in for the reference's importance_generation.py (:8-60).

Same flags (--dataset --data_dir --batch_size --pretrain_dir --limit --net), same output:
importance_score/<net>_limit<L>/*.npy under the current directory, which prune_cifar10.py /
prune_imagenet.py / prune_u2netp.py read through --imp_score. The DCT+score arithmetic runs
in libdctscore (HIP, gfx950); a GPU is required.

Extra, opt-in flags: --synthetic (seeded synthetic batches; also lifts the need for a checkpoint), --input_size,
--seed, --single_sweep, --device_accumulate, --deferred, --criterion (what is scored and where it goes:
the DCT energy under importance_score/, HRank's feature-map rank under rank_conv/, the DCT energy of K frequency bands
per channel, --bands K --band_kind {square,diag}, under band_score/, the spectral entropy of the DCT coefficients
under entropy_score/, or every map's summed distance to the other maps of its layer, the geometric-median criterion, under
gm_score/; --gm_metric {l2,cosine,correlation} takes that distance between the maps as they are or between unit maps, which
go to gm_score/<net>_limit<L>_<metric>/, and --gm_pairs writes the [c, c] matrix of mean pair distances per file instead of its
row sums, to gm_score/<net>_limit<L>[_<metric>]_pairs/, which `python -m dct_pruning_amd.pairs --matrix DIR --rule
{sum,nn,kcenter} --out DIR2` turns into imp_*.npy on the host, and --gm_lowpass K takes every distance between the maps' K x K
lowest DCT coefficients instead of the maps, to gm_score/<net>_limit<L>[_<metric>]_low<K>[_pairs]/; a speed-up for the six
classification nets, a slow-down for u2netp, whose hook shapes have no fused signature kernel), --autocast {fp16,bf16} (the forward sweeps run under torch.autocast and the
half-precision feature maps are scored as they are) and --channels_last (the net and its inputs run in
torch.channels_last and the feature maps are scored in the layout they arrive in). dct_pruning_amd/harness.py says
what each criterion writes and which of these modes and nets it supports (its criterion table and check_options, which
also rejects the command lines here). Multi-GPU: launch with
`python -m torch.distributed.run --nproc-per-node G importance_generation.py ...` — hook points
are sharded over the ranks and rank 0 writes the files.
"""
import argparse
import os
import torch

from dct_pruning_amd import bands, harness, nets


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Importance Assessment")
    parser.add_argument("--dataset", type=str, default="cifar10", choices=("cifar10", "imagenet", "DUTS", "synthetic"),
                        help="dataset")
    parser.add_argument("--data_dir", type=str, default="./data", help="path to dataset")
    parser.add_argument("--batch_size", type=int, default=128, help="batch size")
    parser.add_argument("--pretrain_dir", type=str, default="checkpoints/googlenet.pt",
                        help="load the model from the specified checkpoint")
    parser.add_argument("--limit", type=int, default=5, help="The num of batch to get importence score.")
    parser.add_argument("--net", type=str, default="googlenet",
                        choices=("resnet_50", "vgg_16_bn", "resnet_56", "resnet_110", "densenet_40", "googlenet", "u2netp"),
                        help="net type")
    parser.add_argument("--synthetic", action="store_true", help="seeded synthetic batches of the dataset's shape")
    parser.add_argument("--input_size", type=int, default=None, help="override H=W of synthetic inputs")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--single_sweep", action="store_true", help="score every hook point in one sweep")
    parser.add_argument("--device_accumulate", action="store_true", help="keep the running mean on the GPU")
    parser.add_argument("--deferred", action="store_true",
                        help="single sweep, one scoring launch per tile shape per batch (implies the two above)")
    parser.add_argument("--criterion", type=str, default="dct", choices=harness.CRITERIA,
                        help="dct: DCT energy (importance_score/); rank: HRank feature-map rank (rank_conv/); "
                             "bands: DCT energy per frequency band (band_score/); "
                             "entropy: spectral entropy of the DCT coefficients (entropy_score/); "
                             "gm: summed distance to the other maps of the layer, geometric median (gm_score/)")
    parser.add_argument("--bands", type=int, default=4, help="--criterion bands: number of bands K, 1 ... %d" % bands.BAND_MAX)
    parser.add_argument("--band_kind", type=str, default="square", choices=("square", "diag"),
                        help="--criterion bands: L-infinity shells (square) or anti-diagonal stripes (diag)")
    parser.add_argument("--gm_metric", type=str, default="l2", choices=harness._TABLE["gm"].metrics,
                        help="--criterion gm: l2 compares the maps as they are; cosine (x / |x|) and correlation "
                             "((x - mean) / |x - mean|) compare unit maps, so a channel's gain is no distance and a scaled "
                             "copy is a duplicate (gm_score/<net>_limit<L>_<metric>/)")
    parser.add_argument("--gm_pairs", action="store_true",
                        help="--criterion gm: write the [c, c] matrix of mean pair distances per file instead of its row sums "
                             "(gm_score/<net>_limit<L>[_<metric>]_pairs/); python -m dct_pruning_amd.pairs turns it into "
                             "imp_*.npy under a selection rule (sum, nn, kcenter)")
    parser.add_argument("--gm_lowpass", type=int, default=0,
                        help="--criterion gm: compare the K x K lowest DCT coefficients of the maps instead of the maps, so that "
                             "maps which share their coarse structure are close (0: whole maps; not 1 with correlation; "
                             "gm_score/<net>_limit<L>[_<metric>]_low<K>[_pairs]/). Fast for square maps of edge <= 64 that "
                             "have a codelet; other shapes (u2netp's 72 ... 288) take the dct2d coefficient path and run "
                             "SLOWER than plain gm")
    parser.add_argument("--autocast", type=str, default=None, choices=("fp16", "bf16"),
                        help="run the forward sweeps under torch.autocast and score the half-precision feature maps natively")
    parser.add_argument("--channels_last", action="store_true",
                        help="run the net and its inputs in torch.channels_last and score the feature maps in that layout")
    args = parser.parse_args(argv)
    try:
        harness.check_options(args.criterion, args.net, args.deferred, args.autocast, args.channels_last,
                              (args.bands, args.band_kind), gm_metric=args.gm_metric, gm_pairs=args.gm_pairs,
                              gm_lowpass=args.gm_lowpass)
    except ValueError as e:
        parser.error(str(e))
    return args


load_checkpoint = nets.load_checkpoint  # python -m dct_pruning_amd.prune reads checkpoints the same way


def main(argv=None):
    # before the first HIP call: this pool's driver only supports dmabuf IPC, RCCL fails with hipIpcGetMemHandle otherwise
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("importance_generation.py needs a GPU: the score path has no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # DCTS_REHEARSE=1: every rank on cuda:0 with a gloo group (to rehearse the sharded path on a
    # one-GPU box); normal runs use one GPU per rank and RCCL
    rehearse = os.environ.get("DCTS_REHEARSE") == "1"
    dev = torch.device("cuda", 0 if rehearse else local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from dct_pruning_amd import sharding
        # bounded bring-up: a rank that cannot reach the others prints {"error": ...} and exits 3 (sharding.py)
        sharding.init_process_group("gloo" if rehearse else "nccl", device=dev, what="importance_generation.py")

    torch.manual_seed(args.seed)
    net = nets.get_network(args.net)
    if args.pretrain_dir and os.path.isfile(args.pretrain_dir):
        print("==> Resuming from checkpoint..")
        load_checkpoint(net, args)
        print("Completed! ")
    elif args.synthetic:
        print("==> --synthetic without a checkpoint: random-init weights (seed %d)" % args.seed)
    else:
        print("please speicify a pretrain model ")
        raise NotImplementedError
    net = net.to(dev)

    harness.imp_score(net, args, single_sweep=args.single_sweep,
                      accumulate="device" if args.device_accumulate else "host", deferred=args.deferred,
                      criterion=args.criterion, bands=(args.bands, args.band_kind), autocast=args.autocast,
                      channels_last=args.channels_last, gm_metric=args.gm_metric, gm_pairs=args.gm_pairs,
                      gm_lowpass=args.gm_lowpass)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
