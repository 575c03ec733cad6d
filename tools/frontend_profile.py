"""Driver for a kernel trace of KeypointFrontend.extract: 200 calls at 480 x 640, K = 1024, B images of seeded
random logits and fp16 descriptors (tools/frontend_ab.py's inputs). Run it under the profiler, in a run of
its own, and keep the statistics:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/frontend_profile.py B

(profiles/frontend/kernel_stats_b1.csv, kernel_stats_b16.csv)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")]
import torch  # noqa: E402

from lightglue_amd import KeypointFrontend  # noqa: E402


def main():
    if not torch.cuda.is_available():
        sys.exit("frontend_profile.py: needs a GPU")
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(500 + b)
    logits = torch.randn((b, 65, 60, 80), generator=gen).to(dev)
    dense = torch.randn((b, 256, 60, 80), generator=gen).half().to(dev)
    fe = KeypointFrontend(max_keypoints=1024)
    for _ in range(200):
        fe.extract(logits, dense)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
