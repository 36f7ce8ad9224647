"""Child-process body of tests/test_gpu_crowd_matching.py::test_matching_replays_from_a_graph_on_new_contents.

umi.matching.crowd_match + distance_match are captured once in a HIP graph on static buffers (dot lists, centres and BOTH
count vectors) and replayed after the buffers were overwritten with other cases of other sizes: every replay must give the
new contents' results, because the kernels read the counts on the device and nothing is frozen at capture.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import gen_golden_crowd_matching as G  # noqa: E402
from umi import matching as M  # noqa: E402

DEV = "cuda"
CAP = 512


def lists(names):
    dots = np.zeros((len(names), M.MAX_DOTS, 2), dtype=np.int32)
    centers = np.zeros((len(names), CAP, 2), dtype=np.int32)
    g_count, c_count = np.zeros(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.int32)
    for n, name in enumerate(names):
        g, x, y = G.case(name)
        d, k = M.dot_lists_numpy(g)
        dots[n], g_count[n], c_count[n] = d[0], k[0], x.size
        centers[n, :x.size, 0], centers[n, :x.size, 1] = x, y
    return dots, g_count, centers, c_count


def main():
    assert torch.cuda.is_available()
    rounds = [["random_512", "lattice_64", "empty_dots"], ["more_centres", "random_768", "duplicates"],
              ["empty_both", "border_96x130", "more_dots"]]
    first = lists(rounds[0])
    bufs = [torch.from_numpy(a).to(DEV) for a in first]
    M.match_tables(G.SIGMAS, G.THRESHOLDS, bufs[0].device)

    def step():
        return (M.crowd_match(bufs[0], bufs[1], bufs[2], bufs[3], G.SIGMAS, G.THRESHOLDS),
                M.distance_match(bufs[0], bufs[1], bufs[2], bufs[3], 10))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crowd, dist = step()
    for names in rounds[1:] + rounds[:1]:
        host = lists(names)
        for b, a in zip(bufs, host):
            b.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        want_c = M.crowd_match_numpy(host[0], host[1], host[2], host[3], G.SIGMAS, G.THRESHOLDS)
        want_d = M.distance_match_numpy(host[0], host[1], host[2], host[3], 10)
        assert np.array_equal(crowd.cpu().numpy(), want_c), names
        assert np.array_equal(dist.cpu().numpy(), want_d), names
        print(names, "tp/fp at sigma 5, 0.5:", crowd[:, 0, 0].cpu().tolist(), "distance:", dist.cpu().tolist())
    print("MATCHING_GRAPH_OK")


if __name__ == "__main__":
    main()
