"""The Levenberg-Marquardt policy both optimisers share (csrc/cs_lm.h) against the float64 transcription of g2o's loop in tests/pgo_ref.py.

tools/microbench/lm_policy_check.cpp drives cs_lm.h over fixed sequences of trial results (currentChi, tempChi, scale term, solved) the way
cs_ba_optimize and cs_pgo_optimize do, and prints every input beside what the policy made of it.  Here the printed inputs are replayed
through pgo_ref.Graph.optimize -- the loop itself, not a second copy of it: a Graph whose linearisation, solve and chi2 are scripted.
  * H = diag(max |H_jj|, 0, ...): the loop takes lambda's first value from it, and (H + lambda I)[1, 1] is lambda itself, which is how
    the script sees the lambda of every trial;
  * the loop computes a trial's scale term as sum x (lambda x + b).  With b[1] = 2^200 and x[1] = scale 2^-200 the term lambda x[1]
    (below 2^-54 of b[1] for any lambda < 2^300 / |scale|) is absorbed by the sum and x[1] b[1] = scale exactly;
  * a failed factorisation is cholesky_solve returning None, which is where the loop sets its chi2 and its scale term aside.
lambda must agree to 2 ulp (both sides call the C library's pow); rho, the verdicts, the trial counts, the chi2 and where the run stops
must agree exactly.  ni is not visible in the reference: it is checked through what it does (a rejected trial's lambda is the lambda
before it times the program's ni, exactly) and is 2 after every accepted trial."""
import functools
import math
import os
import subprocess

import numpy as np

import pgo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2.0 ** 200


@functools.lru_cache(maxsize=None)
def _program_output():
    src = os.path.join(ROOT, "tools", "microbench", "lm_policy_check.cpp")
    exe = os.path.join(ROOT, "build_tmp", "lm_policy_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", src, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout


def _parse(text):
    seqs = []
    for line in text.splitlines():
        w = line.split()
        if w[0] == "seq":
            seqs.append(dict(name=w[1], user_lambda=float.fromhex(w[2]), max_diag=float.fromhex(w[3]), max_trials=int(w[4]), asked=int(w[5]), iters=[]))
        elif w[0] == "step":
            it = int(w[1])
            if it == len(seqs[-1]["iters"]):
                seqs[-1]["iters"].append(dict(current=float.fromhex(w[2]), steps=[]))
            assert w[6] == "->"
            seqs[-1]["iters"][it]["steps"].append(dict(current=float.fromhex(w[2]), temp=float.fromhex(w[3]), scale=float.fromhex(w[4]), solved=w[5] == "1",
                                                       rho=float.fromhex(w[7]), accepted=w[8] == "1", lam=float.fromhex(w[9]), ni=float.fromhex(w[10]),
                                                       current_out=float.fromhex(w[11])))
        else:
            assert w[0] == "iter" and int(w[1]) == len(seqs[-1]["iters"]) - 1
            seqs[-1]["iters"][-1].update(trials=int(w[2]), chi=float.fromhex(w[3]), lam=float.fromhex(w[4]), n_bad=int(w[5]), stop=w[6] == "1")
    return seqs


class _Scripted(pgo_ref.Graph):
    """pgo_ref.Graph with one free vertex (n = 7) whose linearisations and trials come from a parsed sequence."""

    def __init__(self, seq):
        one = np.array([[0, 0, 0, 1, 0, 0, 0, 1.0]] * 2)
        super().__init__(one, [1, 0], None, [0], [1], one[:1])
        assert self.n == 7
        self.user_lambda_init, self.max_trials = seq["user_lambda"], seq["max_trials"]
        self.seq, self.it, self.step, self.lams_in = seq, -1, None, []

    def build_system(self):
        self.it += 1
        self.trial = 0
        H, b = np.zeros((7, 7)), np.zeros(7)
        H[0, 0], b[1] = self.seq["max_diag"], BIG
        return H, b, np.float64(self.seq["iters"][self.it]["current"])      # (past the last scripted iteration: IndexError, the test fails)

    def solve(self, A, b):
        self.step = self.seq["iters"][self.it]["steps"][self.trial]
        self.trial += 1
        self.lams_in.append(float(A[1, 1]))
        if not self.step["solved"]:
            return None
        x = np.zeros(7)
        x[1] = self.step["scale"] / BIG
        return x

    def update(self, x):
        pass

    def chi2(self):
        return np.float64(self.step["temp"]), None


def _ulps(a, b):
    return abs(a - b) / math.ulp(b)


def test_policy_matches_the_reference_loop(monkeypatch):
    seqs = _parse(_program_output())
    assert [s["name"] for s in seqs] == ["accept", "reject_to_max", "failed", "inf_positive_rho", "negative_scale", "rho_zero", "bad_iterations"]
    for seq in seqs:
        G = _Scripted(seq)
        monkeypatch.setattr(pgo_ref, "cholesky_solve", G.solve)
        with np.errstate(all="ignore"):
            done = G.optimize(seq["asked"])
        what = seq["name"]
        # where the run stops: the program's last iteration is the reference's, and it says "stop" exactly where fewer were run than asked for
        assert done == len(seq["iters"]), (what, done)
        assert [it["stop"] for it in seq["iters"]] == [False] * (done - 1) + [done < seq["asked"]], what
        assert G.trials_hist == [it["trials"] for it in seq["iters"]], what
        assert [float(c) for c in G.chi2_hist] == [it["chi"] for it in seq["iters"]], what
        steps = [s for it in seq["iters"] for s in it["steps"]]
        assert [r for rhos in G.rho_log for r in rhos] == [s["rho"] for s in steps], what
        # lambda after every step: what the reference's next trial was damped with, and its last value
        lam_ref = G.lams_in[1:] + [float(G.lambda_hist[-1])]
        assert len(lam_ref) == len(steps), what
        lam0 = seq["user_lambda"] if seq["user_lambda"] > 0 else 1e-5 * seq["max_diag"]
        assert G.lams_in[0] == lam0, what
        lam_before, ni_before = lam0, 2.0
        for k, (s, lr) in enumerate(zip(steps, lam_ref)):
            assert _ulps(s["lam"], lr) <= 2, (what, k, s["lam"], lr)
            assert s["accepted"] == (lr < G.lams_in[k]), (what, k)      # (the reference's verdict: an accepted trial lowers lambda, a rejected one raises it)
            if s["accepted"]:
                assert s["ni"] == 2.0 and s["current_out"] == s["temp"], (what, k)
            else:
                assert s["lam"] == lam_before * ni_before and s["ni"] == 2 * ni_before and s["current_out"] == s["current"], (what, k)
            lam_before, ni_before = s["lam"], s["ni"]
        for it, lam_it in zip(seq["iters"], G.lambda_hist):
            assert _ulps(it["lam"], float(lam_it)) <= 2, what


def test_sequences_cover_the_cases():
    """What the sequences are there for, read off the program's own output."""
    seqs = {s["name"]: s for s in _parse(_program_output())}
    steps = lambda n: [s for it in seqs[n]["iters"] for s in it["steps"]]
    third = 1.0 / 3.0
    acc = steps("accept")
    assert all(s["accepted"] for s in acc) and acc[0]["rho"] < 0.5 < acc[1]["rho"]
    ratios = [acc[0]["lam"] / (1e-5 * seqs["accept"]["max_diag"])] + [b["lam"] / a["lam"] for a, b in zip(acc, acc[1:])]
    assert abs(ratios[0] - 2 * third) < 1e-15 and abs(ratios[1] - 2 * third) < 1e-15 and third < ratios[2] < 2 * third and abs(ratios[3] - third) < 1e-15
    r = seqs["reject_to_max"]
    assert r["iters"][-1]["trials"] == r["max_trials"] and r["iters"][-1]["stop"] and len(r["iters"]) < r["asked"]
    f = steps("failed")
    assert [s["solved"] for s in f[:2]] == [False, False] and all(s["scale"] < 0 and not s["accepted"] and s["rho"] == -math.inf for s in f[:2])
    assert math.isinf(f[2]["temp"]) and f[2]["solved"] and not f[2]["accepted"] and f[3]["accepted"]
    p = steps("inf_positive_rho")[0]
    assert p["rho"] == math.inf and not p["accepted"]
    assert steps("negative_scale")[0]["rho"] < 0 < steps("negative_scale")[0]["current"] - steps("negative_scale")[0]["temp"]
    z = seqs["rho_zero"]
    assert steps("rho_zero")[0]["rho"] == 0 and z["iters"][0]["stop"] and len(z["iters"]) == 1
    assert [it["n_bad"] for it in seqs["bad_iterations"]["iters"]] == [1, 2, 0, 1, 2, 3] and seqs["bad_iterations"]["iters"][-1]["stop"]
