ms() { python -c "import json,sys; print(round(json.loads(sys.stdin.read().strip().splitlines()[-1])['ms_per_step'],4))"; }
B="python bench.py --no-cpu-baseline --no-roofline --steps 30"
echo "== forced comm path (1-rank RCCL), eager; calibrated exchange stream"
for i in 1 2; do
 a=$(timeout -k 10 150 $B --force-comm 2>/dev/null | ms)
 g=$(timeout -k 10 150 $B 2>/dev/null | ms)
 echo "graph-nocomm $g | comm path $a"
done
echo "== distill 128^3"
for i in 1 2; do a=$(timeout -k 10 150 $B --workload distill --size 128 2>/dev/null | ms); b=$(timeout -k 10 150 $B --workload distill --size 128 --serial-forwards 2>/dev/null | ms); echo "overlap $a  serial $b"; done
python - <<'P'
import torch, multimodal_segmentation_project_amd as mi
from multimodal_segmentation_project_amd.trainer import concurrent_stream
for i in range(3):
    s = concurrent_stream(torch.device("cuda",0))
    print("concurrent_stream ->", s, getattr(s,"mi3d_overlap_us",None), getattr(s,"mi3d_concurrent",None))
P
