"""Record tests/golden/kernel_stats_families.json: the kernel_stats() table
{config: {family: [launches, bytes, flops]}} that
tests/test_kernel_stats_gpu.py compares against.  Run on a GPU, on the commit
whose bookkeeping is the reference:

    python tools/record_kernel_stats.py [out.json]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import test_kernel_stats_gpu as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    table = {name: t.stats_table(cfg) for name, cfg in t.CONFIGS.items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
