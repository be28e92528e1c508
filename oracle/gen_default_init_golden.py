"""TEST INFRASTRUCTURE ONLY — golden for the default initialisation: what the reference's own `Score(cfg.score)` followed by
`Compressor(cfg.compressor)` draw after `torch.manual_seed(7)` at the tiny config (tests/golden/tiny_cfg.json).

    python oracle/gen_default_init_golden.py     # writes tests/golden/default_init.json

The drop-in classes must consume the generator in the same order and produce the same bits, so the fixture keeps, per module
and in state_dict order, each entry's name, shape, dtype and the SHA-256 of its bytes: bit-equality is all the test asks, and
5 MB of random weights need not be stored to ask it.
"""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_import as R  # noqa: E402
from oracle.gen_golden import OUT  # noqa: E402

SEED = 7


def to_ns(d):
    return SimpleNamespace(**{k: (to_ns(v) if isinstance(v, dict) else v) for k, v in d.items()})


def digest(sd):
    """[[name, shape, dtype, sha256 of the contiguous bytes], ...] in state_dict order"""
    return [[k, list(v.shape), str(v.dtype).replace("torch.", ""), hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()]
            for k, v in sd.items()]


def main():
    R.setup()
    from model.scorenet.score import Score
    from model.Compressor.Network import Compressor
    with open(os.path.join(OUT, "tiny_cfg.json")) as f:
        cfg = to_ns(json.load(f))
    torch.manual_seed(SEED)
    score = Score(cfg.score)
    comp = Compressor(cfg.compressor)
    path = os.path.join(OUT, "default_init.json")
    with open(path, "w") as f:                                      # one state_dict entry per line
        f.write('{"seed": %d' % SEED)
        for name, module in (("score", score), ("compressor", comp)):
            f.write(',\n"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(e) for e in digest(module.state_dict()))))
        f.write("\n}\n")
    print("wrote %-28s %7.1f KB" % ("default_init.json", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
