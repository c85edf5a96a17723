"""CPU: the north-star "drops into pipeline/train/instruction_following.py
unchanged" claim, executed.  The reference's own training script is imported with `shim/` in front of it on sys.path, so its
`from src.otter_ai.models.otter.modeling_otter import OtterForConditionalGeneration` (:49) resolves to otter_amd; third-party
modules that are not installed here and that the Otter branch never calls (deepspeed, wandb, peft, the webdataset loader) are
stubbed.  Then the reference's `train_one_epoch` (:116-251) -- its own masking(), forward_pass(), accelerate backward, clip,
optimizer / scheduler stepping -- drives a tiny OtterForConditionalGeneration for two optimizer steps, and the resulting weights
are compared with otter_amd.train.TrainStep on the same batches.

There is no GPU here and the product has no CPU path, so the arithmetic of the fusion modules comes from the numpy oracle through
tests/_cpu_backend.py (test infrastructure): what this test pins is the CONTRACT -- import path, constructor, attributes the loop
reads (`lang_encoder.__class__.__name__`, `transformer.wte`, `.dtype`, `config.save_pretrained`), forward signature and `[0]` = loss,
parameter names seen by the reference's get_grouped_params / get_checkpoint / mask_embedding.

Where the reference checkout is present (OTTER_REF_ROOT) its script runs live.  Everywhere else what it produced -- losses, a seeded sample
and the update norm of every trained tensor, checkpoint keys -- stands in, recorded by oracle/gen_golden_dropin.py in
tests/golden/dropin_reference_loop.npz, and otter_amd's side of each comparison runs unchanged against it."""
import importlib
import importlib.machinery
import os
import sys
import types
import zlib

import numpy as np
import pytest
import torch

REF = os.environ.get("OTTER_REF_ROOT", "/root/reference")     # (the GPU leg stages the five pipeline/train files elsewhere: tools/stage_reference_loop.sh)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAVE_REF = os.path.isdir(os.path.join(REF, "pipeline", "train"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_reference_loop.npz")
N_SAMPLE = 256        # recorded elements per tensor


def install_reference_script():
    """Import the reference's pipeline/train/instruction_following.py with shim/ in front of it and the uninstalled third-party modules
    stubbed; returns (module, restore) -- shared by the fixture below and by tests/_dropin_ddp_worker.py (one process per rank)."""
    import accelerate  # noqa: F401  (real)
    import transformers  # noqa: F401
    # everything the script pulls from transformers is resolved BEFORE the stubs go in: transformers probes for deepspeed / peft with
    # importlib.util.find_spec while its lazy modules load, and a stub would read as "installed"
    import transformers.trainer_utils  # noqa: F401
    from transformers import (AutoProcessor, AutoTokenizer, CLIPImageProcessor, FuyuImageProcessor, LlamaForCausalLM,  # noqa: F401
                              get_constant_schedule_with_warmup, get_cosine_schedule_with_warmup, get_linear_schedule_with_warmup)
    try:
        from transformers import IdeficsForVisionText2Text  # noqa: F401
        import transformers.models.idefics.processing_idefics  # noqa: F401
    except Exception:
        pass

    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    for name in ("deepspeed", "wandb", "peft"):
        m = types.ModuleType(name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        sys.modules[name] = m
    sys.modules["peft"].LoraConfig = sys.modules["peft"].TaskType = sys.modules["peft"].PeftModel = object
    sys.modules["peft"].get_peft_model = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("peft is not installed"))
    data = types.ModuleType("pipeline.mimicit_utils.data")          # the webdataset / torchvision loader: replaced by synthetic batches
    data.get_data = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError)
    sys.modules["pipeline.mimicit_utils.data"] = data
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    sys.path[:0] = [os.path.join(ROOT, "shim"), ROOT, REF]

    def restore():
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]

    try:
        return importlib.import_module("pipeline.train.instruction_following"), restore
    except BaseException:
        restore()
        raise


@pytest.fixture(scope="module")
def ref_script():
    mod, restore = install_reference_script()
    try:
        yield mod
    finally:
        restore()


class _Loader:
    """What train_one_epoch needs of a MIMIC-IT dataloader: len(), .dataset, iteration over collated batches
    (mimicit_dataset.py collate: net_input = {patch_images [B,T_img,F,3,H,W], input_ids, attention_masks})."""

    def __init__(self, batches):
        self.batches = batches
        self.dataset = list(range(sum(b["net_input"]["input_ids"].shape[0] for b in batches)))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield {"net_input": dict(b["net_input"]), "task_group": list(b["task_group"])}


def _batches(model, n, seed0):
    from oracle import synth

    tok = model.text_tokenizer
    ans, eoc = tok.encode("<answer>")[-1], model.eoc_token_id
    out = []
    for i in range(n):
        vision_x, ids, mask, _ = synth.tiny_batch(seed0 + i)
        ids = ids.copy()
        ids[:, 5] = ans
        ids[:, 11] = eoc
        out.append({"net_input": {"patch_images": torch.from_numpy(vision_x), "input_ids": torch.from_numpy(ids),
                                  "attention_masks": torch.from_numpy(mask)}, "task_group": ["synthetic"] * ids.shape[0]})
    return out


def _build():
    from oracle import synth
    from tests import _golden as G
    from tests.test_host_contract import tiny_model

    model = tiny_model()
    m = G.meta()["otter_tiny"]
    sd = synth.state_dict_for(m["seed"], {k: tuple(v) for k, v in m["state_dict_shapes"].items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def summarize(named):
    """What the fixture keeps of trained weights: per tensor a seeded sample of N_SAMPLE elements (indices from the name) and the norm of the
    update against the initial weights of _build()."""
    init = dict(_build().named_parameters())
    names = sorted(named)
    samples, l2 = [], []
    for n in names:
        w = named[n].detach().reshape(-1).double()
        idx = np.sort(np.random.default_rng([7, zlib.crc32(n.encode())]).choice(w.numel(), min(w.numel(), N_SAMPLE), replace=False))
        samples.append(w[torch.from_numpy(idx)].numpy())
        l2.append(float((w - init[n].detach().reshape(-1).double()).norm()))
    return {"names": np.array(names), "samples": np.concatenate(samples).astype(np.float32), "l2": np.array(l2)}


def recorded(tag):
    with np.load(GOLDEN) as z:
        return {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(tag + ".")}


def assert_weights_match(rec, named):
    """Trained weights against a recorded reference run, at the tolerance of the live comparison (rtol 1e-5, atol 2e-6 per element)."""
    got = summarize(named)
    assert got["names"].tolist() == rec["names"].tolist()
    bad = ~np.isclose(got["samples"], rec["samples"], rtol=1e-5, atol=2e-6)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got["samples"] - rec["samples"]).max()))
    n = np.array([named[k].numel() for k in got["names"]], dtype=np.float64)
    assert np.all(np.abs(got["l2"] - rec["l2"]) <= 1e-5 * rec["l2"] + 2e-6 * np.sqrt(n)), got["names"][np.argmax(np.abs(got["l2"] - rec["l2"]))]


def reference_train_one_epoch(IF, mask_lm_head, tmp_path):
    """The reference's train_one_epoch on otter_amd's model for two steps; returns (trained model, losses, path of the reference's checkpoint)."""
    import otter_amd.modeling_otter as MO
    from accelerate import Accelerator
    from tests._cpu_backend import oracle_backend

    # the reference script's names are otter_amd's classes
    assert IF.OtterForConditionalGeneration is MO.OtterForConditionalGeneration
    assert IF.FlamingoForConditionalGeneration is MO.OtterForConditionalGeneration
    tu = sys.modules["pipeline.train.train_utils"]

    model = _build()
    batches = _batches(model, 2, seed0=11)
    args = types.SimpleNamespace(model_name="otter", total_training_steps=2, gradient_accumulation_steps=1, rank=0, world_size=1, batch_size=2,
                                 remove_answer_token=False, remove_eos_token=False, mask_lm_head=mask_lm_head, distributed_type="NO",
                                 report_to_wandb=False, save_steps_interval=-1, logging_steps=1, num_epochs=1, external_save_dir=str(tmp_path),
                                 save_hf_model=False)
    accelerator = Accelerator(gradient_accumulation_steps=1, mixed_precision="no", cpu=True)
    lr, wd = 1e-3, 0.1
    optimizer = torch.optim.AdamW(tu.get_grouped_params(model, wd=wd), lr=lr)      # the reference's grouping rule on otter_amd's names
    sched = IF.get_constant_schedule_with_warmup(optimizer, num_warmup_steps=0)
    losses = []
    orig_forward = model.forward

    def recording_forward(*a, **k):
        out = orig_forward(*a, **k)
        losses.append(float(out[0].detach()))
        return out

    model.forward = recording_forward
    with oracle_backend():
        IF.train_one_epoch(args, model, 0, [_Loader(batches)], model.text_tokenizer, optimizer, sched, accelerator.device, accelerator, sys.modules["wandb"])
    model.forward = orig_forward
    # the reference's own checkpoint writer on the trained model
    # (the reference pins an older accelerate whose Accelerator.save took `is_main_process`; the installed one does not)
    accelerator.save = lambda obj, f, is_main_process=True, **k: torch.save(obj, f)
    tu.save_final_weights(model, args, accelerator)
    assert os.path.exists(os.path.join(str(tmp_path), "config.json"))
    return model, losses, os.path.join(str(tmp_path), "final_weights.pt")


@pytest.mark.parametrize("mask_lm_head", [False, True])
def test_reference_train_one_epoch_drives_otter_amd(request, mask_lm_head, tmp_path):
    from otter_amd import train as TR
    from tests._cpu_backend import oracle_backend

    lr, wd = 1e-3, 0.1
    if HAVE_REF:
        model, losses, ref_ckpt = reference_train_one_epoch(request.getfixturevalue("ref_script"), mask_lm_head, tmp_path)
        ref_keys = sorted(torch.load(ref_ckpt, map_location="cpu"))
    else:
        rec = recorded("train_one_epoch_mask%d" % int(mask_lm_head))
        losses, ref_keys = rec["losses"].tolist(), rec["ckpt_keys"].tolist()
    assert len(losses) == 2 and all(np.isfinite(losses))

    # the same two steps through otter_amd's own TrainStep (torch AdamW on CPU, fp32, clip 1.0)
    batches = _batches(_build(), 2, seed0=11)
    twin = _build()
    tok = twin.text_tokenizer
    ans = tok.encode("<answer>")[-1]
    step = TR.TrainStep(twin, lr=lr, weight_decay=wd, max_grad_norm=1.0, autocast_dtype=None, hip_optimizer=False,
                        mask_lm_head=mask_lm_head, answer_token_id=ans)
    twin_losses = []
    with oracle_backend():
        for b in batches:
            ni = b["net_input"]
            labels = TR.masking(ni["input_ids"], ans, twin.eoc_token_id, tok.encode(tok.eos_token)[-1])
            twin_losses.append(float(step(ni["patch_images"], ni["input_ids"], ni["attention_masks"], labels)))
    assert np.allclose(losses, twin_losses, rtol=1e-6, atol=0), (losses, twin_losses)
    # (TrainStep adds the lookup rows of the tied embedding after the dense un-embedding gradient instead of as a second dense tensor: the
    #  clipping coefficient moves in its last bit, and AdamW's m / (sqrt(v) + eps) turns that into up to lr * O(1e-3) on elements whose
    #  gradient is of the order of eps -- hence the absolute term)
    if HAVE_REF:
        for (n, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
            assert torch.allclose(a, b, rtol=1e-5, atol=2e-6), (n, float((a - b).abs().max()))
    else:
        assert_weights_match(rec, dict(twin.named_parameters()))
    assert losses[1] != losses[0]

    # the reference's own checkpoint writer on the trained model == otter_amd.train's (same keys, same tensors)
    ours = TR.get_checkpoint(twin)
    assert ref_keys == sorted(ours)
    if not HAVE_REF:
        model, ref_ckpt = twin, os.path.join(str(tmp_path), "final_weights.pt")
        torch.save(ours, ref_ckpt)
    fresh = _build()
    TR.load_trained_ckpt(fresh, ref_ckpt)
    for (n, a), (_, b) in zip(model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n


def reference_forward_pass(IF):
    """forward_pass (:73-103) on the tiny model and batch 3; returns (its loss, the model's own loss on the same inputs)."""
    from oracle import synth
    from tests._cpu_backend import oracle_backend

    model = _build()
    vision_x, ids, mask, labels = (torch.from_numpy(a) for a in synth.tiny_batch(3))
    args = types.SimpleNamespace(model_name="otter")
    with oracle_backend():
        loss = IF.forward_pass(args, model, model.text_tokenizer, vision_x, ids, mask, labels, "cpu", torch.float32, {})
        want = model(vision_x=vision_x, lang_x=ids, attention_mask=mask, labels=labels).loss
    return loss, want


def test_reference_forward_pass_signature(request):
    """forward_pass (:73-103) calls model(vision_x=images.to(autocast_type), lang_x=, attention_mask=, labels=)[0]."""
    if HAVE_REF:
        loss, want = reference_forward_pass(request.getfixturevalue("ref_script"))
        assert loss.ndim == 0 and float(loss) == float(want)
        return
    from oracle import synth
    from tests._cpu_backend import oracle_backend

    rec = recorded("forward_pass")
    model = _build()
    vision_x, ids, mask, labels = (torch.from_numpy(a) for a in synth.tiny_batch(3))
    with oracle_backend():
        want = model(vision_x=vision_x.to(torch.float32), lang_x=ids, attention_mask=mask, labels=labels)[0]
    assert int(rec["loss_ndim"]) == 0 and want.ndim == 0
    assert np.isclose(float(want), float(rec["loss"]), rtol=1e-6, atol=0), (float(want), float(rec["loss"]))


def reference_ddp_run(tmp_path):
    """Two processes (torch.distributed.run, gloo, CPU) run tests/_dropin_ddp_worker.py; returns rank 0's blob."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="2", OTTER_REF_ROOT=REF)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "_dropin_ddp_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return torch.load(os.path.join(str(tmp_path), "ddp_rank0.pt"), map_location="cpu")


def test_reference_loop_under_accelerate_ddp(tmp_path):
    """The same drop-in under `accelerate`'s DistributedDataParallel (VERDICT r2 missing #4): two processes (torch.distributed.run, gloo, CPU),
    each runs the reference's own main()-style sequence -- Accelerator(), accelerator.prepare(model, optimizer, scheduler), train_one_epoch with
    its own two batches -- on otter_amd's model through shim/ (tests/_dropin_ddp_worker.py).  Rank 0's trained weights must equal a
    single-process computation that averages the two ranks' gradients by hand (DDP's contract), clips at 1.0 and takes the AdamW step."""
    from otter_amd import train as TR
    from tests._cpu_backend import oracle_backend

    if HAVE_REF:
        blob = reference_ddp_run(tmp_path)
        world, wrapped, ref_losses = blob["world"], blob["wrapped"], blob["losses"]
    else:
        rec = recorded("ddp")
        world, wrapped, ref_losses = int(rec["world"]), str(rec["wrapped"]), rec["losses"].tolist()
    assert world == 2 and wrapped == "DistributedDataParallel" and len(ref_losses) == 2

    # expected: per step, the mean of the two ranks' gradients -> clip_grad_norm_(1.0) -> AdamW with the reference's parameter groups
    # (the reference's get_grouped_params where its checkout is present, otter_amd.train's restatement of it elsewhere)
    restore = None
    if HAVE_REF:
        _, restore = install_reference_script()
    try:
        twin = _build()
        if HAVE_REF:
            groups = sys.modules["pipeline.train.train_utils"].get_grouped_params(twin, wd=0.1)
            mine = TR.get_grouped_params(twin, 0.1)
            assert [([id(p) for p in g["params"]], g["weight_decay"]) for g in groups] == [([id(p) for p in g["params"]], g["weight_decay"]) for g in mine]
        else:
            groups = TR.get_grouped_params(twin, 0.1)
        tok = twin.text_tokenizer
        ans, eos = tok.encode("<answer>")[-1], tok.encode(tok.eos_token)[-1]
        opt = torch.optim.AdamW(groups, lr=1e-3)
        per_rank = [_batches(twin, 2, seed0=11 + 100 * r) for r in range(2)]
        params = [p for p in twin.parameters() if p.requires_grad]
        want_losses = []
        with oracle_backend():
            for step in range(2):
                acc = [torch.zeros_like(p) for p in params]
                for r in range(2):
                    ni = per_rank[r][step]["net_input"]
                    labels = TR.masking(ni["input_ids"], ans, twin.eoc_token_id, eos)
                    loss = twin(vision_x=ni["patch_images"], lang_x=ni["input_ids"], attention_mask=ni["attention_masks"], labels=labels)[0]
                    if r == 0:
                        want_losses.append(float(loss.detach()))
                    for a, g in zip(acc, torch.autograd.grad(loss, params)):
                        a += g / 2
                for p, a in zip(params, acc):
                    p.grad = a
                torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
                opt.step()
                opt.zero_grad()
    finally:
        if restore is not None:
            restore()
    assert np.allclose(ref_losses, want_losses, rtol=1e-6), (ref_losses, want_losses)
    named = {n: p for n, p in twin.named_parameters() if p.requires_grad}
    if not HAVE_REF:
        assert_weights_match(rec, named)
        return
    got = blob["weights"]
    assert sorted(got) == sorted(named)
    for n, p in named.items():
        assert torch.allclose(got[n], p.detach(), rtol=1e-5, atol=2e-6), (n, float((got[n] - p.detach()).abs().max()))
