#!/usr/bin/env python3
"""The reference's saved test-environment sets as the files themselves, for tests/test_testsets_cpu.py: the joblib pickles
(algos/multiagent/evaluation/test_environments/test_env_dict_obs<k>_<snr>_v4, written by
algos/test_environment/eval/test_env_gen.py:13-69) are what radiation_ppo_amd.testsets parses, so the reader is pinned to the
original bytes, not to a re-encoding.  Keeping all 32 sets (15 MB) is not needed: the archive holds the names of every set
(MANIFEST) and the bytes of the sample the test parses (every sixth set in name order, plus obs1_none), xz-compressed.

    python tests/golden/make_testset_files.py <reference root>   ->  tests/golden/testset_files.tar.xz
"""
import io
import os
import sys
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "testset_files.tar.xz")


def sample(names):
    """The sets tests/test_testsets_cpu.py parses, from the sorted list of every set name."""
    return names[::6] + [x for x in names if "obs1_none" in x]


def main(ref):
    root = os.path.join(ref, "algos", "multiagent", "evaluation", "test_environments")
    names = sorted(f for f in os.listdir(root) if f.startswith("test_env_dict_obs") and f.endswith("_v4"))

    def add(tar, name, data):
        info = tarfile.TarInfo(name)
        info.size = len(data)                       # mtime / uid / gid stay 0: the archive depends on the bytes only
        tar.addfile(info, io.BytesIO(data))

    with tarfile.open(OUT, "w:xz", preset=9) as tar:
        add(tar, "MANIFEST", "".join(n + "\n" for n in names).encode())
        for n in sample(names):
            with open(os.path.join(root, n), "rb") as f:
                add(tar, n, f.read())
    print(len(names), "sets,", len(sample(names)), "stored ->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
