# round-3 evidence run C (GPU box): the default bench line once the PMC record carries this binary's hash (roofline.traffic non-null),
# and the full-configuration score / mask parity records (tests/mask_parity.py: identical activations scored by the GPU path and by the
# CPU oracle) for ResNet-50 and U2-Net-p at 288 and 320
# usage: bash tools/final_r03_c.sh <output dir>
d=${1:?usage: bash tools/final_r03_c.sh <output dir>}
export TMPDIR=/tmp
mkdir -p "$d"
python bench.py --full > $d/bench_default.json 2> $d/bench_default.err || { tail $d/bench_default.err; exit 1; }
python tests/mask_parity.py --net u2netp --batch_size 12 --limit 5 --input_size 288 --out $d/mask_u2netp_288.txt > $d/mask_u2netp_288.log 2>&1 || { tail $d/mask_u2netp_288.log; exit 1; }
tail -3 $d/mask_u2netp_288.txt
python tests/mask_parity.py --net u2netp --batch_size 12 --limit 5 --input_size 320 --out $d/mask_u2netp_320.txt > $d/mask_u2netp_320.log 2>&1 || { tail $d/mask_u2netp_320.log; exit 1; }
tail -3 $d/mask_u2netp_320.txt
python tests/mask_parity.py --net resnet_50 --batch_size 256 --limit 5 --out $d/mask_resnet50.txt > $d/mask_resnet50.log 2>&1 || { tail $d/mask_resnet50.log; exit 1; }
tail -3 $d/mask_resnet50.txt
