"""Generates tests/golden/exchange_bytes.json: for the partitioned scenarios of
tests/test_exchange_bytes_gpu.py, every rank's received exchange bytes and
transport call count over the whole run.  Needs the product library and a GPU
(the ranks share it through gloo).  Record it with the library whose wire
format is the one to pin.  Usage: python tests/golden/make_golden_exchange.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "go-libp2p-pubsub_amd"))
sys.path.insert(0, TESTS)

import test_exchange_bytes_gpu as xb  # noqa: E402


def main():
    path = os.path.join(HERE, "exchange_bytes.json")
    res = {name: {"world": world, "ranks": xb.measure(world, name)} for world, name in xb.CASES}
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))
    print("wrote", path)


if __name__ == "__main__":
    main()
