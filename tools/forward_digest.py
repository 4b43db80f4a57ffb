"""tools/forward_digest.py <libA.so> <libB.so>  -- bit-for-bit comparison of the 16-bit forward and of training of two builds of the
library (files that `python -m mapf_gpt_amd.build --out` writes): one SHA-256 of the output bytes per case, side by side, and a verdict.

The case list is fixed here: seeded synthetic weights and tokens.  Forward: every released shape, two shapes of the packed / generic chains
and the one-layer variants; both precisions; small calls, large calls with and without a remainder chunk, an uneven persistent grid, the
sequence forward and act_tokens.  Training (TRAIN_MODELS, chunks of 2 rows, targets half -1 with one row all -1): per precision the loss and
every gradient after a one-chunk call, a call of chunks 2, 2, 1 and an accumulating call, then after an f32 call followed by a bf16 call;
each time the total norm of clip_grad_norm_(1.0) and the state_dict() after one AdamW step; then the loss and every gradient of
forward_backward_rows, of forward_backward under config.dropout = 0.1 (all four sites, set_dropout_rng pinned, row0 = 3) and of
forward_backward_rows_drop with the same masks, each per precision as a one-chunk call of 2 rows and a 5-row call in chunks 2, 2, 1.
Every (library, environment setting, model) runs in a fresh process, with MGPT_LIB_PATH naming the library, under its own time limit; the
first process that fails ends the run.  A refactor of the host side must leave the two columns identical.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {  # name -> model_args
    "tiny": "tiny", "2M": "2M", "6M": "6M", "85M": "85M",
    "c256h4": dict(n_layer=2, n_head=4, n_embd=256), "c512h8": dict(n_layer=2, n_head=8, n_embd=512),
    "tiny_L1": dict(n_layer=1, n_head=2, n_embd=64), "2M_L1": dict(n_layer=1, n_head=5, n_embd=160), "6M_L1": dict(n_layer=1, n_head=8, n_embd=256),
}
# (environment setting, models, precisions): one process each per model
GROUPS = [({}, list(MODELS), ("f16x3", "bf16")),
          ({"MGPT_L0_TABLE": "0"}, ["6M"], ("f16x3", "bf16")),
          ({"MGPT_LN_FOLD": "0"}, ["85M"], ("bf16",))]
TRAIN_MODELS = ("tiny", "2M", "6M", "85M")    # head size 32, and 64 (85M); one process each
TIME_LIMIT = 420    # seconds per process


def child(model, precisions):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from mapf_gpt_amd.model import build_model

    tokens = np.random.default_rng(5).integers(0, 67, size=(600, 256), dtype=np.uint8)
    targets = np.random.default_rng(6).integers(-1, 67, size=(130, 256), dtype=np.int64)
    dev = torch.from_numpy(tokens).cuda()

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    for precision in precisions:
        def net(max_rows):
            return build_model(MODELS[model], seed=3, scale=2.0, max_rows=max_rows, precision=precision, envelope="ignore")
        tag = f"{model} {precision}"
        n = net(256)
        for rows in (1, 40, 128, 129, 200):                       # small calls; large calls in one chunk
            print(f"{tag} max_rows=256 rows={rows} logits {digest(n.logits_tokens(dev[:rows].contiguous()))}", flush=True)
        for rows in (3, 130):
            logits, _ = n.forward(dev[:rows].contiguous(), torch.from_numpy(targets[:rows]))
            print(f"{tag} max_rows=256 rows={rows} forward_seq {digest(logits)}", flush=True)
        for rows in (40, 200):
            print(f"{tag} max_rows=256 rows={rows} act_tokens {digest(n.act_tokens(dev[:rows].contiguous(), do_sample=False))}", flush=True)
        del n
        n = net(128)
        for rows in (129, 200):                                   # large calls in chunks of 128: remainders of 1 and 72 rows
            print(f"{tag} max_rows=128 rows={rows} logits {digest(n.logits_tokens(dev[:rows].contiguous()))}", flush=True)
        del n
        if model in ("2M", "6M"):                                 # more rows than compute units, and no multiple of them
            n = net(600)
            print(f"{tag} max_rows=600 rows=600 logits {digest(n.logits_tokens(dev))}", flush=True)
            del n


def child_train(model):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from mapf_gpt_amd import weights
    from mapf_gpt_amd.model import build_model

    rng = np.random.default_rng(7)
    tokens = torch.from_numpy(rng.integers(0, 67, size=(10, 256), dtype=np.uint8)).cuda()
    targets = rng.integers(0, 67, size=(10, 256)).astype(np.int64)
    targets[rng.random((10, 256)) < 0.5] = -1
    targets[[1, 6]] = -1                                          # rows with no targeted position
    targets = torch.from_numpy(targets)
    net = build_model(model, seed=3, max_rows=2).train(max_rows=2)
    opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95))

    def digest(tag, *tensors):                                    # (named_parameters order for gradients and parameters)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        print(f"{model} train {tag} {h.hexdigest()}", flush=True)

    def step(tag, calls):                                         # calls: (precision, first row, rows) into one gradient buffer
        net.zero_grad()
        for i, (precision, r0, n) in enumerate(calls):
            loss = net.forward_backward(tokens[r0:r0 + n].contiguous(), targets[r0:r0 + n], precision=precision)
            digest(f"{tag} call {i} {precision} rows={n} loss+grads", loss, *net.grads().values())
        digest(f"{tag} total norm", net.clip_grad_norm_(1.0))
        opt.step()
        sd = net.state_dict()
        digest(f"{tag} state_dict", *(sd[n] for n, _ in net.named_parameters()))

    for precision in ("f32", "bf16"):
        step(f"{precision} one chunk", [(precision, 0, 2)])
        step(f"{precision} chunks 2,2,1 then accumulate", [(precision, 0, 5), (precision, 5, 5)])
    step("f32 then bf16", [("f32", 0, 2), ("bf16", 2, 5)])

    # the last-position micro-step and dropout: per call and precision a one-chunk call of 2 rows and a 5-row call in chunks 2, 2, 1 (a
    # remainder chunk, the call's row advancing across chunks, the bf16 compact matrix padded to 32 > rows), into zeroed gradients
    labels = torch.from_numpy(rng.integers(0, 67, size=10).astype(np.int64))     # (drawn last: the cases above keep their data)

    def micro_steps(n, tag, call):
        for precision in ("f32", "bf16"):
            for r0, rows in ((0, 2), (2, 5)):
                n.zero_grad()
                loss = call(slice(r0, r0 + rows), precision)
                digest(f"{tag} {precision} rows={rows} loss+grads", loss, *n.grads().values())

    micro_steps(net, "rows", lambda r, precision: net.forward_backward_rows(tokens[r].contiguous(), labels[r], precision=precision))
    del net, opt
    nd = build_model(dict(weights.model_args(model), dropout=0.1), seed=3, max_rows=2)
    nd.set_dropout_rng(11)
    nd.train(max_rows=2)
    drop = dict(dropout_step=4, row0=3, dropout_sites=15)         # all four sites; the masks pinned, the call's first row not row 0
    micro_steps(nd, "dropout 0.1", lambda r, precision: nd.forward_backward(tokens[r].contiguous(), targets[r], precision=precision, **drop))
    micro_steps(nd, "rows dropout 0.1", lambda r, precision: nd.forward_backward_rows_drop(tokens[r].contiguous(), labels[r], precision=precision, **drop))


def run(lib_path):
    lib_path = os.path.abspath(lib_path)
    name = os.path.basename(lib_path)
    lines = []

    def one(env, model, *child_args):
        cmd = ["timeout", "-k", "10", str(TIME_LIMIT), sys.executable, os.path.abspath(__file__), *child_args]
        r = subprocess.run(cmd, env=dict(os.environ, MGPT_LIB_PATH=lib_path, **env), capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"forward_digest: {name} {env} {child_args[0]} {model}: exit status {r.returncode}; nothing more is started")
        prefix = " ".join(f"{k}={v}" for k, v in env.items())
        print(f"# {name} {prefix} {child_args[0]} {model}: done", file=sys.stderr, flush=True)
        lines.extend((prefix + " " + ln).strip() for ln in r.stdout.splitlines() if " " in ln and len(ln.rsplit(" ", 1)[1]) == 64)

    for env, models, precisions in GROUPS:
        for model in models:
            one(env, model, "--child", model, ",".join(precisions))
    for model in TRAIN_MODELS:
        one({}, model, "--child-train", model)
    return lines


def main():
    if len(sys.argv) >= 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3].split(","))
    if len(sys.argv) >= 2 and sys.argv[1] == "--child-train":
        return child_train(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = run(sys.argv[1]), run(sys.argv[2])
    differing = 0
    print(f"{'case':<80} {sys.argv[1]:<64} {sys.argv[2]:<64}")
    for la, lb in zip(a, b):
        (ca, ha), (cb, hb) = la.rsplit(" ", 1), lb.rsplit(" ", 1)
        same = ca == cb and ha == hb
        differing += 0 if same else 1
        print(f"{ca:<80} {ha} {hb}{'' if same else '  <-- DIFFERS'}")
    differing += abs(len(a) - len(b))
    print(f"{len(a)} / {len(b)} cases, differing {differing}")
    sys.exit(1 if differing or not a else 0)


if __name__ == "__main__":
    main()
