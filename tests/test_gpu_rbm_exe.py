"""GPU: gen_rand_net -> BPpretrain_RBM -> BPtrain_Sigmoid on the original project's 10-sentence sample (tests/golden/
tools_pfile*) with a tiny net.  The .wts BPpretrain_RBM writes holds the bits of the Python session (BPGpu.rbm) driven
with the same chunks and seeds -- the trainer's own host IO gives the chunk order and the rows -- and BPtrain_Sigmoid
starts from it and logs a finite CV."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hostlib

pytestmark = pytest.mark.gpu
DIM, CTX, B, TOFF = 257, 3, 32, 1
LS = [DIM * CTX, 48, 40, DIM]
SEED, EPOCHS = 27870775, 2
RBM = dict(rbm_epochs=EPOCHS, rbm_lrate_gauss=0.002, rbm_lrate=0.02, momentum=0.5, weightcost=0.0002)


def run(exe, cwd, kv):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([os.path.join(hostlib.HOST, exe)] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True,
                          text=True, timeout=300, cwd=cwd)


def test_gen_rand_net_pretrain_finetune(pkg, tmp_path):
    d = tmp_path
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    sample = hostlib.sample_pfiles(d / "tools_pfile")
    subprocess.check_call([os.path.join(hostlib.HOST, "gen_rand_net"), str(len(LS)), *map(str, LS), str(d), str(d / "init.wts"),
                           "1", "1.0", "7"], stdout=subprocess.DEVNULL)
    io_kv = dict(gpu_used=0, numlayers=len(LS), layersizes=",".join(map(str, LS)), bunchsize=B, fea_dim=DIM, fea_context=CTX,
                 traincache=500, init_randem_seed=SEED, targ_offset=TOFF, initwts_file=d / "init.wts",
                 norm_file=os.path.join(sample, "train_noisy.norm"), fea_file=os.path.join(sample, "train_noisy.pfile"),
                 targ_file=os.path.join(sample, "train_clean.pfile"), train_sent_range="0-7", cv_sent_range="8-9")
    # 1. the tool, under the names the issue gives three of its keys
    kv = dict(io_kv, outwts_file="pre.wts", log_file="pre.log", **RBM)
    for alias, key in (("train_pfile_name", "fea_file"), ("train_cache_frames", "traincache"), ("train_cache_seed", "init_randem_seed")):
        kv[alias] = kv.pop(key)
    res = run("BPpretrain_RBM", d / "pre", kv)
    assert res.returncode == 0 and "all finish!" in res.stdout, res.stdout + res.stderr
    log = open(d / "pre" / "pre.log").read()
    errs = {(int(l), int(e)): float(v) for l, e, v in re.findall(
        r"^RBM layer (\d) \(\w+\) epoch (\d) of 2: mean reconstruction error per frame ([\d.]+) over \d+ frames$", log, re.M)}
    assert sorted(errs) == [(1, 1), (1, 2), (2, 1), (2, 2)], log
    assert all(math.isfinite(v) and v > 0 for v in errs.values())
    assert re.search(r"RBM layer 1 \(gaussian\)", log) and re.search(r"RBM layer 2 \(bernoulli\)", log)

    # 2. the same chunks and seeds through the Python session
    w0, b0 = hostlib.read_wts(str(d / "init.wts"), LS)
    io = hostlib.HostIO(**dict(io_kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    eng = pkg.BPGpu(SEED, 0, LS, B, 0.1, 0.9, 1e-5, w0, b0, 2.0, 0)
    got = {}
    try:
        starts, _ = io.plan(io_kv["train_sent_range"])
        assert len(starts) >= 3
        for layer, vis, lr in ((1, "gaussian", RBM["rbm_lrate_gauss"]), (2, "bernoulli", RBM["rbm_lrate"])):
            with eng.rbm(layer, vis, lrate=lr, momentum=RBM["momentum"], weightcost=RBM["weightcost"], seed=SEED) as rbm:
                for ep in range(1, EPOCHS + 1):
                    sq = frames = 0
                    for ci in io.shuffle(len(starts)):
                        inp, _ = io.read_chunk(ci, LS[0], DIM, 600)
                        n, s = rbm.train(inp)
                        sq, frames = sq + s, frames + n * B
                    got[(layer, ep)] = sq / frames
        we, be = eng.returnWeights()
    finally:
        io.close()
        eng.close()
    ws, bs = hostlib.read_wts(str(d / "pre" / "pre.wts"), LS)
    for l in range(3):
        assert np.array_equal(ws[l].view(np.uint32), we[l].view(np.uint32)), l
        assert np.array_equal(bs[l].view(np.uint32), be[l].view(np.uint32)), l
    for l in (0, 1):
        assert not np.array_equal(ws[l], w0[l])                       # pre-training moved the hidden layers
    assert np.array_equal(ws[2], w0[2]) and np.array_equal(bs[2], b0[2])    # ... and never the output layer
    for k, v in errs.items():
        assert abs(v - got[k]) <= 1e-6 * max(1.0, abs(got[k])), (k, v, got[k])      # the log prints six decimals

    # 3. the trainer starts from it
    kv = dict(io_kv, initwts_file=d / "pre" / "pre.wts", outwts_file="mlp.wts", log_file="mlp.log", MLflag=1, shapefactor=1.2,
              lrate=0.1, momentum=0.9, weightcost=1e-5, dropoutflag=0, visible_omit=0.1, hid_omit=0.1)
    res = run("BPtrain_Sigmoid", d / "fine", kv)
    assert res.returncode == 0 and "all finish!" in res.stdout, res.stdout + res.stderr
    m = re.search(r"^CV over\. squared error: (-?[\d.]+)$", open(d / "fine" / "mlp.log").read(), re.M)
    assert m and math.isfinite(float(m.group(1))) and float(m.group(1)) > 0
    assert os.path.getsize(d / "fine" / "mlp.wts") == os.path.getsize(d / "pre" / "pre.wts")

    # 4. a layer that is not hidden is refused before anything is trained
    res = run("BPpretrain_RBM", d / "bad", dict(io_kv, outwts_file="pre.wts", log_file="pre.log", rbm_layers="1,3", **RBM))
    assert res.returncode != 0 and "rbm_layers: layer 3 is not a hidden layer 1..2" in res.stderr
