#!/usr/bin/env python3
"""Generate golden input/output vectors by running the REFERENCE implementation on CPU.

Runs ONLY in the authoring container (needs /root/reference).  The reference's Python never
travels to the GPU box; only the .npz files written here do.  Re-run:

    python tests/golden/make_golden.py

What is executed (all f32, CPU, torch.manual_seed fixed):
  * protnote/models/protein_encoders.py  ProteInfer.get_embeddings / forward   (eval + train-mode BN)
  * protnote/models/ProtNote.py          ProtNote.forward for the 4 FEATURE_FUSION modes,
                                         eval (with and without description ensembling) and train
  * protnote/utils/losses.py             BCE / FocalLoss through get_loss
  * protnote/models/ProtNoteTrainer.py   calculate_tp_fn_fp / calculate_f1 / calculate_f1_micro and the
                                         body of the train step (:728-755): loss -> backward ->
                                         clip_grad_norm_(1.0) -> Adam(lr=3e-4).step()
  * protnote/data/collators.py           collate_variable_sequence_length
  * protnote/data/datasets.py            ProteinDataset label-index bookkeeping on a toy FASTA (vocabularies,
                                         multihots, embedding-row filter/sort/sample) - integer, bit-exact
  * inspect.signature of the reference objects tests/test_signatures.py compares against (JSON), and
    configs/base_config.yaml re-dumped as plain data (tests/test_config_surface.py)

Absent third-party modules that are NOT on the arithmetic path are stubbed in sys.modules.
torchvision.ops.MLP (pinned torchvision==0.15.2 in the reference's setup.py:17) is absent from this
image; its constructor is restated below (a pure nn.Sequential builder; the arithmetic is torch.nn).
"""
import os
import sys
import types
import importlib.machinery

import numpy as np
import torch

REF = os.environ.get("PROTNOTE_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, k):
        return _Anything()


def install_stubs():
    import transformers  # noqa: F401  (must be imported before a fake torchvision exists)

    class MLP(torch.nn.Sequential):
        """torchvision.ops.MLP (v0.15.2) constructor, restated."""

        def __init__(self, in_channels, hidden_channels, norm_layer=None,
                     activation_layer=torch.nn.ReLU, inplace=None, bias=True, dropout=0.0):
            params = {} if inplace is None else {"inplace": inplace}
            layers = []
            in_dim = in_channels
            for hidden_dim in hidden_channels[:-1]:
                layers.append(torch.nn.Linear(in_dim, hidden_dim, bias=bias))
                if norm_layer is not None:
                    layers.append(norm_layer(hidden_dim))
                layers.append(activation_layer(**params))
                layers.append(torch.nn.Dropout(dropout, **params))
                in_dim = hidden_dim
            layers.append(torch.nn.Linear(in_dim, hidden_channels[-1], bias=bias))
            layers.append(torch.nn.Dropout(dropout, **params))
            super().__init__(*layers)

    tv = _stub("torchvision")
    tv.ops = _stub("torchvision.ops", MLP=MLP)
    bio = _stub("Bio")
    bio.SeqIO = _stub("Bio.SeqIO")
    bio.ExPASy = _stub("Bio.ExPASy", Enzyme=_Anything())
    _stub("Bio.Seq", Seq=_Anything)
    _stub("Bio.SeqRecord", SeqRecord=_Anything)
    _stub("blosum", BLOSUM=lambda n: {})
    _stub("wget")
    _stub("pynvml", nvmlInit=_Anything(), nvmlDeviceGetHandleByIndex=_Anything(),
          nvmlDeviceGetMemoryInfo=_Anything())
    _stub("loralib", Linear=_Anything)
    _stub("wandb")
    tm = _stub("torchmetrics", MetricCollection=_Anything, Metric=object)
    tm.classification = _stub("torchmetrics.classification", Precision=_Anything, Recall=_Anything,
                              BinaryPrecision=_Anything, BinaryRecall=_Anything, F1Score=_Anything,
                              AveragePrecision=_Anything)
    te = _stub("torcheval")
    te.metrics = _stub("torcheval.metrics", MultilabelAUPRC=_Anything, BinaryAUPRC=_Anything,
                       BinaryBinnedAUPRC=_Anything, MultilabelBinnedAUPRC=_Anything, Mean=_Anything,
                       BinaryF1Score=_Anything)
    te.metrics.toolkit = _stub("torcheval.metrics.toolkit", sync_and_compute=_Anything())
    sys.path.insert(0, REF)


def randomize_(module, g):
    """Randomise BN affine/running stats and rescale weights so activations/logits are O(1)
    (default init gives logits ~ -0.0105 +- 5e-4, which would make a 1e-3 tolerance vacuous)."""
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
        elif isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
            with torch.no_grad():
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.6 / fan_in ** 0.5))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)


def sd_np(module, prefix=""):
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def onehots(g, lens, lmax, pad_garbage=False):
    b = len(lens)
    x = torch.zeros(b, 20, lmax)
    ids = torch.randint(0, 20, (b, lmax), generator=g)
    x.scatter_(1, ids[:, None, :], 1.0)
    for i, n in enumerate(lens):
        x[i, :, n:] = 7.0 if pad_garbage else 0.0
    return x, ids


# --------------------------------------------------------------------------------------------
def golden_encoder():
    from protnote.models.protein_encoders import ProteInfer

    g = torch.Generator().manual_seed(1234)
    cfg = dict(num_labels=13, input_channels=20, output_channels=52, kernel_size=9,
               dilation_base=3, num_resnet_blocks=5, bottleneck_factor=0.5)
    torch.manual_seed(0)
    model = ProteInfer(activation=torch.nn.ReLU, **cfg)
    randomize_(model, g)
    out = {"cfg_" + k: np.array(v) for k, v in cfg.items()}
    out.update(sd_np(model, "sd/"))

    lens = [200, 1, 37, 150, 199, 9]
    lmax = 200
    x, ids = onehots(g, lens, lmax, pad_garbage=True)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    out["x"] = x.numpy()
    out["lens"] = lens_t.numpy()

    model.eval()
    with torch.no_grad():
        feats = model.conv1(x, lens_t)
        out["eval/conv1"] = feats.numpy().copy()
        for i, blk in enumerate(model.resnet_blocks):
            feats = blk(feats, lens_t)
            if i in (0, 4):
                out[f"eval/block{i}"] = feats.numpy().copy()
        out["eval/embeddings"] = model.get_embeddings(x, lens_t).numpy()
        out["eval/logits"] = model(x, lens_t).numpy()
        # pad-length invariance: same sequences padded to 260 with zeros
        x2 = torch.zeros(len(lens), 20, 260)
        x2[:, :, :lmax] = x
        for i, n in enumerate(lens):
            x2[i, :, n:] = 0.0
        out["eval/embeddings_pad260"] = model.get_embeddings(x2, lens_t).numpy()

    # train-mode BN: frozen encoder still uses batch stats and updates buffers
    model.train()
    with torch.no_grad():
        out["train/embeddings"] = model.get_embeddings(x, lens_t).numpy()
    out.update(sd_np(model, "sd_after_train/"))
    np.savez_compressed(os.path.join(OUT, "encoder_small.npz"), **out)
    print("encoder_small.npz", {k: v.shape for k, v in out.items() if not k.startswith("sd")})


# --------------------------------------------------------------------------------------------
def _train_step(model, loss_fn, inputs, targets, clip=1.0, lr=3e-4):
    """Body of ProtNoteTrainer.train_one_epoch :728-755 on CPU (autocast/GradScaler are no-ops)."""
    from torch.nn.utils import clip_grad_norm_

    params = [p for n, p in model.named_parameters()
              if p.requires_grad and not n.startswith("sequence_encoder")]
    opt = torch.optim.Adam(params, lr=lr)
    logits, _ = model(**inputs)
    loss = loss_fn(logits, targets.float())
    loss.backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()
             if p.grad is not None}
    total_norm = clip_grad_norm_(model.parameters(), max_norm=clip)
    opt.step()
    opt.zero_grad()
    return logits.detach().numpy().copy(), float(loss.detach()), grads, float(total_norm)


def golden_encoder_pieces():
    """MaskedConv1D.forward and Residual.forward called STAND-ALONE (protein_encoders.py:8-17, :61-67) - the two public
    classes under ProteInfer - on inputs whose pad positions hold garbage, which is what tells a stand-alone call from the
    fused pipeline: MaskedConv1D masks before and after; Residual normalises the RAW input (train-mode BatchNorm statistics
    include the pads) and adds it back unmasked, so its output carries the input's pad values.  Same toy model and seeds as
    golden_encoder (the weights are stored again so the fixture is self-contained)."""
    from protnote.models.protein_encoders import ProteInfer

    g = torch.Generator().manual_seed(1234)
    cfg = dict(num_labels=13, input_channels=20, output_channels=52, kernel_size=9,
               dilation_base=3, num_resnet_blocks=5, bottleneck_factor=0.5)
    torch.manual_seed(0)
    model = ProteInfer(activation=torch.nn.ReLU, **cfg)
    randomize_(model, g)
    out = {"cfg_" + k: np.array(v) for k, v in cfg.items()}
    out.update(sd_np(model, "sd/"))
    lens = [120, 1, 37, 90, 119, 9]
    lens_t = torch.tensor(lens, dtype=torch.int64)
    g2 = torch.Generator().manual_seed(4321)
    h = torch.randn(len(lens), 52, 120, generator=g2)  # pads hold random values too
    out["h"], out["lens"] = h.numpy(), lens_t.numpy()
    model.eval()
    with torch.no_grad():
        out["conv/block2_masked_conv1"] = model.resnet_blocks[2].masked_conv1(h, lens_t).numpy()   # 52 -> 26, k 9, dilation 9
        out["conv/block1_masked_conv2"] = model.resnet_blocks[1].masked_conv2(h[:, :26].contiguous(), lens_t).numpy()  # 1 x 1
        out["eval/residual1"] = model.resnet_blocks[1](h, lens_t).numpy()   # dilation 3
        out["eval/residual4"] = model.resnet_blocks[4](h, lens_t).numpy()   # dilation 81 > most lengths
    blk = model.resnet_blocks[1]
    blk.train()
    with torch.no_grad():
        out["train/residual1"] = blk(h, lens_t).numpy()
    for k, v in blk.state_dict().items():
        if "running" in k or "num_batches" in k:
            out["after_train/residual1." + k] = v.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "encoder_pieces.npz"), **out)
    print("encoder_pieces.npz", {k: v.shape for k, v in out.items() if not k.startswith("sd")})


def golden_protnote(variants=None):
    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.losses import get_loss
    import protnote.models.ProtNote as PN

    enc_cfg = dict(num_labels=7, input_channels=20, output_channels=28, kernel_size=9,
                   dilation_base=3, num_resnet_blocks=2, bottleneck_factor=0.5)
    head_cfg = dict(protein_embedding_dim=28, label_embedding_dim=24, latent_dim=16,
                    output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=3,
                    outout_mlp_add_batchnorm=True, projection_head_num_layers=4,
                    projection_head_hidden_dim_scale_factor=3, dropout=0.0,
                    label_embedding_noising_alpha=20.0, temperature=0.07)
    lens = [50, 3, 21, 50, 17, 44]
    lmax = 50
    n_labels = 10
    base_head_cfg = dict(head_cfg)
    if variants is None:
        variants = [(f, True) for f in ("concatenation", "concatenation_diff", "concatenation_prod", "similarity")]
    for fusion, out_bn in variants:
        head_cfg = dict(base_head_cfg, outout_mlp_add_batchnorm=out_bn)  # OUTPUT_MLP_BATCHNORM
        g = torch.Generator().manual_seed(99)
        torch.manual_seed(1)
        enc = ProteInfer(activation=torch.nn.ReLU, **enc_cfg)
        model = ProtNote(sequence_encoder=enc, label_encoder=None, feature_fusion=fusion,
                         inference_descriptions_per_label=2, **head_cfg)
        randomize_(model, g)
        for n, p in model.named_parameters():
            if n.startswith("sequence_encoder"):
                p.requires_grad = False
        out = {"fusion": np.array(fusion)}
        out.update({"enc_cfg_" + k: np.array(v) for k, v in enc_cfg.items()})
        out.update({"head_cfg_" + k: np.array(v) for k, v in head_cfg.items()})
        out.update(sd_np(model, "sd/"))
        x, _ = onehots(g, lens, lmax)
        lens_t = torch.tensor(lens, dtype=torch.int64)
        # 2 descriptions per label, consecutive rows belong to one label (datasets.py:327-343)
        lab = torch.randn(n_labels * 2, 24, generator=g)
        counts = torch.randint(3, 30, (n_labels * 2,), generator=g)
        y = (torch.rand(len(lens), n_labels, generator=g) < 0.3).to(torch.int64)
        out.update(x=x.numpy(), lens=lens_t.numpy(), label_embeddings=lab.numpy(),
                   label_token_counts=counts.numpy(), multihots=y.numpy())

        model.eval()
        with torch.no_grad():
            lg, _ = model(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab)
            out["eval/logits_ens2"] = lg.numpy()          # [B, n_labels] (ensembled, ProtNote.py:313-322)
            model.inference_descriptions_per_label = 1
            lg1, _ = model(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab)
            out["eval/logits_raw"] = lg1.numpy()          # [B, 2*n_labels]
            model.inference_descriptions_per_label = 2
            out["eval/P_f"] = model.sequence_encoder.get_embeddings(x, lens_t).numpy()
            out["eval/P_e"] = model.W_p(torch.from_numpy(out["eval/P_f"])).numpy()
            out["eval/L_e"] = model.W_l(lab).numpy()

        # ---- train step on the first description of each label, fixed noise tensor ----
        lab1 = lab[0::2].contiguous()
        cnt1 = counts[0::2].contiguous()
        u = torch.rand(lab1.shape, generator=g)
        out["train/noise_u"] = u.numpy()
        real_rand_like = torch.rand_like
        PN.torch.rand_like = lambda t, *a, **k: u.clone()
        try:
            for loss_name in ("BCE", "FocalLoss"):
                m2 = type(model)(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg),
                                 label_encoder=None, feature_fusion=fusion,
                                 inference_descriptions_per_label=2, **head_cfg)
                m2.load_state_dict(model.state_dict())
                for n, p in m2.named_parameters():
                    if n.startswith("sequence_encoder"):
                        p.requires_grad = False
                m2.train()
                cfg = {"params": {"LOSS_FN": loss_name, "FOCAL_LOSS_GAMMA": 2, "FOCAL_LOSS_ALPHA": -1,
                                  "LABEL_SMOOTHING": 0.0}}
                loss_fn = get_loss(cfg, bce_pos_weight=torch.tensor(1.0))
                inputs = dict(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab1,
                              label_token_counts=cnt1)
                logits, loss, grads, gnorm = _train_step(m2, loss_fn, inputs, y)
                p = f"train_{loss_name}/"
                out[p + "logits"] = logits
                out[p + "loss"] = np.array(loss, dtype=np.float32)
                out[p + "grad_norm"] = np.array(gnorm, dtype=np.float32)
                for k, v in grads.items():
                    out[p + "grad/" + k] = v
                out.update(sd_np(m2, p + "sd_after/"))
            if fusion == "concatenation":
                # TRAIN_SEQUENCE_ENCODER: True - gradients reach every encoder parameter (ProtNote.py:248-256)
                m3 = type(model)(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg), label_encoder=None,
                                 feature_fusion=fusion, inference_descriptions_per_label=2,
                                 train_sequence_encoder=True, **head_cfg)
                m3.load_state_dict(model.state_dict())
                m3.train()
                loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
                inputs = dict(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab1,
                              label_token_counts=cnt1)
                logits3, _ = m3(**inputs)
                loss3 = loss_fn(logits3, y.float())
                loss3.backward()
                out["train_enc_BCE/loss"] = np.array(float(loss3.detach()), dtype=np.float32)
                out["train_enc_BCE/logits"] = logits3.detach().numpy().copy()
                for n3, p3 in m3.named_parameters():
                    if p3.grad is not None:
                        out["train_enc_BCE/grad/" + n3] = p3.grad.numpy().copy()
        finally:
            PN.torch.rand_like = real_rand_like
        fn = os.path.join(OUT, f"protnote_small_{fusion}{'' if out_bn else '_nobn'}.npz")
        np.savez_compressed(fn, **out)
        print(os.path.basename(fn), os.path.getsize(fn) // 1024, "KiB")


# --------------------------------------------------------------------------------------------
def golden_losses_extra():
    """The reference's other LOSS_FN choices (losses.py:58-170: RGDBCE, CBLoss, WeightedBCE, BatchWeightedBCE)."""
    from protnote.utils.losses import get_loss

    g = torch.Generator().manual_seed(17)
    logits = torch.randn(29, 41, generator=g) * 2.5
    y = (torch.rand(29, 41, generator=g) < 0.15).to(torch.int64)
    y[3] = 0                                   # a protein without positives (zero row weight)
    label_weights = torch.rand(41, generator=g) * 5 + 0.1          # WeightedBCE: inverse-frequency style weights
    label_counts = torch.randint(0, 400, (41,), generator=g).float()  # CBLoss: label frequencies (some zero)
    label_counts[5] = 0
    out = {"logits": logits.numpy(), "multihots": y.numpy(), "label_weights": label_weights.numpy(),
           "label_counts": label_counts.numpy()}
    cases = {"RGDBCE": ({"LOSS_FN": "RGDBCE", "RGDBCE_TEMP": 0.12}, None),
             "RGDBCE_hot": ({"LOSS_FN": "RGDBCE", "RGDBCE_TEMP": 5.0}, None),
             "BatchWeightedBCE": ({"LOSS_FN": "BatchWeightedBCE"}, None),
             "WeightedBCE": ({"LOSS_FN": "WeightedBCE"}, label_weights),
             "CBLoss": ({"LOSS_FN": "CBLoss"}, label_counts),
             # row 3 has no positives: 0 in the loss, NaN in the gradient (losses.py:46-53 nan_to_num + autograd)
             "SupCon": ({"LOSS_FN": "SupCon", "SUPCON_TEMP": 0.07}, None)}
    for name, (params, lw) in cases.items():
        fn = get_loss({"params": params}, label_weights=lw)
        lg = logits.clone().requires_grad_(True)
        l = fn(lg, y.float())
        l.backward()
        out[name + "/loss"] = l.detach().numpy()
        out[name + "/dlogits"] = lg.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "losses_extra.npz"), **out)
    print("losses_extra.npz")


def golden_losses_metrics():
    from protnote.utils.losses import get_loss, FocalLoss
    from protnote.models.ProtNoteTrainer import calculate_tp_fn_fp, calculate_f1, calculate_f1_micro

    g = torch.Generator().manual_seed(7)
    logits = torch.randn(33, 57, generator=g) * 3
    logits[0, 0] = 0.0          # sigmoid == 0.5 == threshold edge (>=)
    logits[1, 1] = 40.0
    logits[2, 2] = -40.0
    y = (torch.rand(33, 57, generator=g) < 0.2).to(torch.int64)
    out = {"logits": logits.numpy(), "multihots": y.numpy()}
    for name, pw in (("BCE", 1.0), ("BCE_pw", 3.5)):
        fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(pw))
        lg = logits.clone().requires_grad_(True)
        l = fn(lg, y.float())
        l.backward()
        out[f"{name}/loss"] = l.detach().numpy()
        out[f"{name}/dlogits"] = lg.grad.numpy()
        out[f"{name}/pos_weight"] = np.array(pw, dtype=np.float32)
    for name, gamma, alpha, ls in (("Focal", 2, -1, 0.0), ("Focal_a", 2, 0.25, 0.0),
                                   ("Focal_ls", 1.5, -1, 0.1)):
        fn = FocalLoss(alpha=alpha, gamma=gamma, label_smoothing=ls)
        lg = logits.clone().requires_grad_(True)
        l = fn(lg, y.float())
        l.backward()
        out[f"{name}/loss"] = l.detach().numpy()
        out[f"{name}/dlogits"] = lg.grad.numpy()
        out[f"{name}/params"] = np.array([gamma, alpha, ls], dtype=np.float32)
    for th in (0.5, 0.3):
        tp, fn_, fp = calculate_tp_fn_fp(torch.sigmoid(logits), y, threshold=th)
        out[f"th{th}/tp"], out[f"th{th}/fn"], out[f"th{th}/fp"] = tp.numpy(), fn_.numpy(), fp.numpy()
        out[f"th{th}/f1"] = calculate_f1(tp, fn_, fp).numpy()
        out[f"th{th}/f1_micro"] = calculate_f1_micro(tp, fn_, fp).numpy()
    np.savez_compressed(os.path.join(OUT, "losses_metrics.npz"), **out)
    print("losses_metrics.npz")


# --------------------------------------------------------------------------------------------
def golden_collator():
    from protnote.data.collators import collate_variable_sequence_length

    g = torch.Generator().manual_seed(5)
    lens = [7, 3, 11, 5]
    n_lab, d = 6, 8
    lab = torch.randn(n_lab, d, generator=g)
    cnt = torch.randint(1, 9, (n_lab,), generator=g)
    batch = []
    out = {}
    for i, n in enumerate(lens):
        ids = torch.randint(0, 20, (n,), generator=g)
        oh = torch.nn.functional.one_hot(ids, 20).T.float()       # [20, n] (datasets.py process_example)
        mh = (torch.rand(n_lab, generator=g) < 0.4).to(torch.int64)
        batch.append({"sequence_onehots": oh, "sequence_id": f"P{i}", "sequence_length": torch.tensor(n),
                      "label_multihots": mh, "label_embeddings": lab, "label_token_counts": cnt})
        out[f"in/ids{i}"] = ids.numpy()
        out[f"in/multihots{i}"] = mh.numpy()
    out["in/label_embeddings"] = lab.numpy()
    out["in/label_token_counts"] = cnt.numpy()
    res = collate_variable_sequence_length(batch, label_sample_size=None, distribute_labels=False,
                                           shuffle_labels=False, in_batch_sampling=False,
                                           grid_sampler=False, world_size=1, rank=0)
    for k, v in res.items():
        if torch.is_tensor(v):
            out["out/" + k] = v.numpy()
            out["out_dtype/" + k] = np.array(str(v.dtype))
        else:
            out["out/" + k] = np.array(v)
    np.savez_compressed(os.path.join(OUT, "collator.npz"), **out)
    print("collator.npz", {k: getattr(v, "shape", None) for k, v in res.items()})




# --------------------------------------------------------------------------------------------
def golden_bookkeeping():
    """Label-index bookkeeping of protnote/data/datasets.py::ProteinDataset (INT, must be bit-exact):
    vocabularies, label2int, multihots, embedding-row filter, min/max index per label, sorted / sampled
    embedding rows.  Runs the reference Dataset on a tiny FASTA + embedding index written to a temp dir."""
    import logging
    import tempfile

    import pandas as pd
    import Bio.SeqIO as SeqIO

    class _Rec:
        def __init__(self, desc, seq):
            self.description, self.seq = desc, seq

    def _parse(path, fmt):
        desc, seq = None, []
        for line in open(path):
            line = line.rstrip("\n")
            if line.startswith(">"):
                if desc is not None:
                    yield _Rec(desc, "".join(seq))
                desc, seq = line[1:], []
            elif line:
                seq.append(line)
        if desc is not None:
            yield _Rec(desc, "".join(seq))

    SeqIO.parse = _parse
    from protnote.data.datasets import ProteinDataset

    fasta = [("P3", "MKTAYIAKQR", ["GO:0003", "GO:0001"]),
             ("P1", "ACDEFGHIKLMNPQRSTVWY", ["GO:0002"]),
             ("P2", "MKTAYIAKQR", ["GO:0009"]),           # duplicate sequence -> dropped by DEDUPLICATE
             ("P4", "GGSGGS", ["GO:0001", "GO:0004", "GO:0002"]),
             ("P5", "WWYV", ["GO:0004"])]
    rows = []
    for gid in ["GO:0004", "GO:0001", "GO:0007", "GO:0002", "GO:0003"]:      # deliberately unsorted, with an unused id
        for dt in ["name", "label", "synonym_exact", "synonym_exact"]:
            rows.append({"id": gid, "description_type": dt, "description": f"{gid}-{dt}-{len(rows)}",
                         "token_count": 3 + len(rows) % 7})
    index = pd.DataFrame(rows)
    emb = torch.arange(len(rows), dtype=torch.float32)[:, None].repeat(1, 4) + 0.25
    out = {"fasta_ids": np.array([f[0] for f in fasta]), "fasta_seqs": np.array([f[1] for f in fasta]),
           "fasta_labels": np.array([" ".join(f[2]) for f in fasta]),
           "index_id": index["id"].values.astype(str), "index_type": index["description_type"].values.astype(str),
           "index_token_count": index["token_count"].values, "embeddings": emb.numpy()}
    real_load = torch.load
    torch.load = lambda *a, **k: real_load(*a, **{**k, "weights_only": False})
    try:
        with tempfile.TemporaryDirectory() as d:
            fp = os.path.join(d, "toy.fasta")
            with open(fp, "w") as f:
                for sid, seq, labs in fasta:
                    f.write(">" + " ".join([sid] + labs) + "\n" + seq + "\n")
            ep = os.path.join(d, "emb.pt")
            torch.save(emb, ep)
            torch.save(index, os.path.join(d, "emb_index.pt"))
            for dtype, aug in (("test", "name+label"), ("train", "name+label+synonym_exact")):
                cfg = {"params": {"AUGMENT_RESIDUE_PROBABILITY": 0.0, "LABEL_AUGMENTATION_DESCRIPTIONS": aug,
                                  "TRAIN_SUBSET_FRACTION": 1, "TEST_SUBSET_FRACTION": 1, "VALIDATION_SUBSET_FRACTION": 1,
                                  "INFERENCE_GO_DESCRIPTIONS": "name+label", "EXTRACT_VOCABULARIES_FROM": None,
                                  "DEDUPLICATE": True, "MAX_SEQUENCE_LENGTH": 15},
                       "paths": {}, "LABEL_EMBEDDING_PATH": ep}
                ds = ProteinDataset({"data_path": fp, "dataset_type": dtype}, cfg, logger=logging.getLogger("g"))
                p = dtype + "/"
                out[p + "kept_ids"] = np.array([r[1] for r in ds.data])
                out[p + "label_vocabulary"] = np.array(ds.label_vocabulary)
                out[p + "amino_acid_vocabulary"] = np.array(ds.amino_acid_vocabulary)
                out[p + "represented_vocabulary_mask"] = np.array(ds.represented_vocabulary_mask)
                out[p + "filtered_rows"] = (ds.label_embeddings[:, 0] - 0.25).long().numpy()   # original row ids
                out[p + "min_idx"] = np.array([ds.label_embeddings_index[g]["min_idx"] for g in ds.label_vocabulary])
                out[p + "max_idx"] = np.array([ds.label_embeddings_index[g]["max_idx"] for g in ds.label_vocabulary])
                out[p + "sorted_rows"] = (ds.sorted_label_embeddings[:, 0] - 0.25).long().numpy()
                out[p + "sorted_token_counts"] = np.asarray(ds.sorted_label_token_counts)
                np.random.seed(123)
                se, sc = ds._sample_label_embeddings()
                out[p + "sampled_rows_seed123"] = (se[:, 0] - 0.25).long().numpy()
                out[p + "sampled_token_counts_seed123"] = np.asarray(sc)
                for i in range(len(ds)):
                    seq, sid, labs = ds.data[i]
                    ex = ds.process_example(seq, sid, labs)
                    out[p + f"ex{i}/onehots"] = ex["sequence_onehots"].numpy()
                    out[p + f"ex{i}/multihots"] = ex["label_multihots"].numpy()
                    out[p + f"ex{i}/length"] = ex["sequence_length"].numpy()
    finally:
        torch.load = real_load
    np.savez_compressed(os.path.join(OUT, "bookkeeping.npz"), **out)
    print("bookkeeping.npz", [k for k in out if k.startswith("test/") and "ex" not in k])


def golden_tf_weights():
    """utils/proteinfer.py:7-41 transfer_tf_weights_to_torch on a synthetic TF-variable pickle (TF layouts:
    conv kernels [k, Cin, Cout], dense [in, out]); the pickle itself is the input fixture."""
    import pickle
    from collections import OrderedDict

    from protnote.models.protein_encoders import ProteInfer
    from protnote.utils.proteinfer import transfer_tf_weights_to_torch

    rng = np.random.RandomState(3)
    cfg = dict(num_labels=6, input_channels=20, output_channels=12, kernel_size=9, dilation_base=3,
               num_resnet_blocks=2, bottleneck_factor=0.5)
    C, Cb, k = 12, 6, 9
    tf = OrderedDict()
    tf["inferrer/conv1d/kernel:0"] = rng.randn(k, 20, C).astype(np.float32)
    tf["inferrer/conv1d/bias:0"] = rng.randn(C).astype(np.float32)
    n = 0
    for blk in range(2):
        for width, kk, cin, cout in ((C, k, C, Cb), (Cb, 1, Cb, C)):
            pre = f"inferrer/residual_block_{blk}/batch_normalization_{n}/"
            tf[pre + "gamma:0"] = rng.rand(width).astype(np.float32) + 0.5
            tf[pre + "beta:0"] = rng.randn(width).astype(np.float32)
            tf[pre + "moving_mean:0"] = rng.randn(width).astype(np.float32)
            tf[pre + "moving_variance:0"] = rng.rand(width).astype(np.float32) + 0.5
            tf[f"inferrer/residual_block_{blk}/conv1d_{n}/kernel:0"] = rng.randn(kk, cin, cout).astype(np.float32)
            tf[f"inferrer/residual_block_{blk}/conv1d_{n}/bias:0"] = rng.randn(cout).astype(np.float32)
            n += 1
    tf["inferrer/logits/kernel:0"] = rng.randn(C, 6).astype(np.float32)
    tf["inferrer/logits/bias:0"] = rng.randn(6).astype(np.float32)
    tf["inferrer/global_step:0"] = np.int64(12345)
    path = os.path.join(OUT, "tf_weights_small.pkl")
    with open(path, "wb") as f:
        pickle.dump(tf, f)
    model = ProteInfer(activation=torch.nn.ReLU, **cfg)
    transfer_tf_weights_to_torch(model, path)
    out = {"cfg_" + k_: np.array(v) for k_, v in cfg.items()}
    out.update(sd_np(model, "sd/"))
    np.savez_compressed(os.path.join(OUT, "tf_weights_small_expected.npz"), **out)
    print("tf_weights_small.pkl + expected", len(out))


def golden_attention_pooling():
    """LABEL_EMBEDDING_POOLING_METHOD: all (ProtNote.py:89-91,154-166,266-267): cached TOKEN embeddings [N, T, d] +
    attention mask -> additive-attention pooled label embeddings (eval), and one train step in which raw_attn_scorer
    is trained (label noise included: for 3-D label embeddings its scale is alpha / sqrt(T), ProtNote.py:227-230)."""
    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.losses import get_loss
    import protnote.models.ProtNote as PN

    enc_cfg = dict(num_labels=7, input_channels=20, output_channels=28, kernel_size=9,
                   dilation_base=3, num_resnet_blocks=2, bottleneck_factor=0.5)
    head_cfg = dict(protein_embedding_dim=28, label_embedding_dim=24, latent_dim=16,
                    output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=3,
                    outout_mlp_add_batchnorm=True, projection_head_num_layers=4,
                    projection_head_hidden_dim_scale_factor=3, dropout=0.0,
                    label_embedding_noising_alpha=20.0, temperature=0.07,
                    label_embedding_pooling_method="all")
    g = torch.Generator().manual_seed(4242)
    torch.manual_seed(3)

    def build():
        m = ProtNote(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg), label_encoder=None,
                     feature_fusion="concatenation", inference_descriptions_per_label=1, **head_cfg)
        for n, p in m.named_parameters():
            if n.startswith("sequence_encoder"):
                p.requires_grad = False
        return m

    model = build()
    randomize_(model, g)
    lens = [50, 3, 21, 50, 17, 44]
    x, _ = onehots(g, lens, 50)
    lens_t = torch.tensor(lens, dtype=torch.int64)
    N, T, d = 9, 11, 24
    hidden = torch.randn(N, T, d, generator=g)
    ntok = torch.tensor([11, 1, 5, 11, 2, 7, 3, 9, 4])
    mask = (torch.arange(T)[None, :] < ntok[:, None]).to(torch.int64)
    y = (torch.rand(len(lens), N, generator=g) < 0.3).to(torch.int64)
    out = {"fusion": np.array("concatenation")}
    out.update({"enc_cfg_" + k: np.array(v) for k, v in enc_cfg.items()})
    out.update({"head_cfg_" + k: np.array(v) for k, v in head_cfg.items()})
    out.update(sd_np(model, "sd/"))
    out.update(x=x.numpy(), lens=lens_t.numpy(), hidden=hidden.numpy(), attention_mask=mask.numpy(),
               token_counts=ntok.numpy(), multihots=y.numpy())
    tok = {"attention_mask": mask}
    model.eval()
    with torch.no_grad():
        out["eval/pooled"] = model.additive_attention(hidden, mask).numpy()
        lg, _ = model(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=hidden, tokenized_labels=tok)
        out["eval/logits"] = lg.numpy()
    u = torch.rand(hidden.shape, generator=g)
    out["train/noise_u"] = u.numpy()
    real_rand_like = torch.rand_like
    PN.torch.rand_like = lambda t, *a, **k: u.clone()
    try:
        m2 = build()
        m2.load_state_dict(model.state_dict())
        m2.train()
        loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
        inputs = dict(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=hidden, tokenized_labels=tok,
                      label_token_counts=ntok)
        logits, loss, grads, gnorm = _train_step(m2, loss_fn, inputs, y)
        out["train_BCE/logits"] = logits
        out["train_BCE/loss"] = np.array(loss, dtype=np.float32)
        out["train_BCE/grad_norm"] = np.array(gnorm, dtype=np.float32)
        for k, v in grads.items():
            out["train_BCE/grad/" + k] = v
        out.update(sd_np(m2, "train_BCE/sd_after/"))
    finally:
        PN.torch.rand_like = real_rand_like
    np.savez_compressed(os.path.join(OUT, "protnote_small_attention.npz"), **out)
    print("protnote_small_attention.npz", sorted(k for k in out if "raw_attn" in k))


def golden_samplers():
    """Index streams of protnote/data/samplers.py::DistributedWeightedSampler (torch.multinomial + randperm on a
    generator seeded with the epoch, rank-strided) for 2 ranks x 2 epochs, with and without replacement."""
    from protnote.data.samplers import DistributedWeightedSampler

    g = torch.Generator().manual_seed(11)
    weights = torch.rand(37, generator=g).double() + 0.05
    out = {"weights": weights.numpy()}
    for repl in (True, False):
        for world in (1, 2):
            for rank in range(world):
                n = 37 if repl else 30  # without replacement the reference needs len(weights) > total_size
                w = weights if repl else torch.cat([weights, weights[:8]])
                s = DistributedWeightedSampler(w, world_size=world, rank=rank, replacement=repl)
                if not repl:
                    s.num_samples = n // world
                    s.total_size = s.num_samples * world
                for epoch in (0, 1):
                    s.set_epoch(epoch)
                    out[f"repl{int(repl)}/w{world}/r{rank}/e{epoch}"] = np.array(list(iter(s)))
    np.savez_compressed(os.path.join(OUT, "samplers.npz"), **out)
    print("samplers.npz", len(out))


def golden_config0_full_width():
    """BASELINE configs[0] shape at the REAL width (ProteInfer 1100 channels / 5 blocks, d = 1024, h = 3072, 4-layer
    projections, 3-layer output MLP): the REFERENCE's object graph (ProteInfer -> ProtNote -> get_loss -> the train-step body
    ProtNoteTrainer.py:728-755 with ONE Adam across the epoch) on tests.helpers.config0_case() - 4 steps, label noise fed
    from the case's seeded draws.  Stored: the loss trajectory, gradient norms, step-1 logits, every BatchNorm buffer after the
    epoch, and for every trained tensor its norm and first 256 entries (the weights themselves are regenerated from the seed)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from tests.helpers import config0_case
    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.losses import get_loss
    import protnote.models.ProtNote as PN
    from torch.nn.utils import clip_grad_norm_

    c = config0_case()
    enc = ProteInfer(activation=torch.nn.ReLU, **c["ecfg"])
    model = ProtNote(sequence_encoder=enc, label_encoder=None, protein_embedding_dim=1100, label_embedding_dim=1024,
                     latent_dim=1024, output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=3,
                     projection_head_num_layers=4, projection_head_hidden_dim_scale_factor=3,
                     label_embedding_noising_alpha=20.0, feature_fusion="concatenation")
    model.load_state_dict(c["sd"])
    for n, p in model.named_parameters():
        if n.startswith("sequence_encoder"):
            p.requires_grad = False
    out = {"losses": [], "grad_norms": []}
    # inference before any training: the 256 label rows read as 128 labels x 2 descriptions, ensembled (ProtNote.py:313-322)
    model.eval()
    model.inference_descriptions_per_label = 2
    with torch.no_grad():
        x0, lens0, _ = c["batch"](0)
        out["eval0/logits_ens2"] = model(sequence_onehots=x0, sequence_lengths=lens0, label_embeddings=c["lab"])[0].numpy().copy()
        out["eval0/P_f"] = model.sequence_encoder.get_embeddings(x0, lens0).numpy().copy()
        model.inference_descriptions_per_label = 1
        out["eval0/logits_raw"] = model(sequence_onehots=x0, sequence_lengths=lens0, label_embeddings=c["lab"])[0].numpy().copy()
    model.inference_descriptions_per_label = 1
    model.train()
    loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=3e-4)
    real = torch.rand_like
    try:
        for k in range(c["n_steps"]):
            x, lens, y = c["batch"](k)
            u = c["noises"][k]
            PN.torch.rand_like = lambda t, *a, **kw: u.clone()
            logits, _ = model(sequence_onehots=x, sequence_lengths=lens, label_embeddings=c["lab"],
                              label_token_counts=c["cnt"])
            loss = loss_fn(logits, y.float())
            loss.backward()
            out["grad_norms"].append(float(clip_grad_norm_(model.parameters(), max_norm=1.0)))
            opt.step()
            opt.zero_grad()
            out["losses"].append(float(loss.detach()))
            if k == 0:
                out["step0/logits"] = logits.detach().numpy().copy()
    finally:
        PN.torch.rand_like = real
    out["losses"] = np.array(out["losses"], dtype=np.float64)
    out["grad_norms"] = np.array(out["grad_norms"], dtype=np.float64)
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["after/buffer/" + k] = v.detach().numpy().copy()
        elif not k.startswith("sequence_encoder"):
            flat = v.detach().reshape(-1)
            out["after/param_head/" + k] = flat[:256].numpy().copy()
            out["after/param_norm/" + k] = np.array(float(flat.double().norm()))
    np.savez_compressed(os.path.join(OUT, "config0_full_width.npz"), **out)
    print("config0_full_width.npz", os.path.getsize(os.path.join(OUT, "config0_full_width.npz")) // 1024, "KiB", out["losses"])


def golden_optimizer_branches():
    """Every branch of ProtNoteTrainer._set_optimizer (ProtNoteTrainer.py:199-245) driven by the REFERENCE'S OWN trainer:
    the real ProtNoteTrainer is constructed from a config dict (so _set_optimizer picks what is frozen and which torch
    optimiser is built) and its real train_one_epoch (:675-825) runs 10 batches - TRAIN_PROJECTION_HEAD True / False x
    OPTIMIZER Adam / AdamW / SGD (WEIGHT_DECAY 0.01), clip 1, label noise fed from seeded draws.  Stored per case: the
    names the reference left trainable, the first batch's logits, every batch's loss, the epoch's train metrics and the
    whole state dict after the epoch.  (torcheval's Mean / sync_and_compute and the torchmetrics collection - absent
    here, off the arithmetic path - are stood in by a running mean and an empty collection.)"""
    import json
    import logging
    import tempfile
    import warnings

    import torch.distributed as dist

    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.losses import get_loss
    import protnote.models.ProtNote as PN
    import protnote.models.ProtNoteTrainer as PT

    class _Mean:
        def __init__(self, device=None):
            self.s, self.n = 0.0, 0

        def update(self, v):
            self.s += float(v)
            self.n += 1

        def compute(self):
            return torch.tensor(self.s / max(self.n, 1))

    class _NoMetrics(dict):
        def reset(self):
            pass

        def __call__(self, *a, **k):
            pass

        def compute(self):
            return {}

    PT.Mean = _Mean
    PT.sync_and_compute = lambda m: m.compute()

    enc_cfg = dict(num_labels=7, input_channels=20, output_channels=28, kernel_size=9,
                   dilation_base=3, num_resnet_blocks=2, bottleneck_factor=0.5)
    head_cfg = dict(protein_embedding_dim=28, label_embedding_dim=24, latent_dim=16,
                    output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=3,
                    outout_mlp_add_batchnorm=True, projection_head_num_layers=4,
                    projection_head_hidden_dim_scale_factor=3, dropout=0.0,
                    label_embedding_noising_alpha=20.0, temperature=0.07)
    g = torch.Generator().manual_seed(2024)
    torch.manual_seed(5)

    def build():
        return ProtNote(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg), label_encoder=torch.nn.Identity(),
                        feature_fusion="concatenation", inference_descriptions_per_label=1, **head_cfg)

    model0 = build()
    randomize_(model0, g)
    n_batches, B, n_labels, lmax = 10, 6, 12, 40
    lab = torch.randn(n_labels, 24, generator=g)
    cnt = torch.randint(3, 30, (n_labels,), generator=g)
    batches, noises = [], []
    for k in range(n_batches):
        lens = torch.randint(1, lmax + 1, (B,), generator=g)
        lens[0] = lmax
        x, _ = onehots(g, lens.tolist(), lmax)
        y = (torch.rand(B, n_labels, generator=g) < 0.3).to(torch.int64)
        batches.append({"sequence_onehots": x, "sequence_lengths": lens, "label_multihots": y, "label_embeddings": lab,
                        "label_token_counts": cnt})
        noises.append(torch.rand(lab.shape, generator=g))

    class _Loader(list):
        pass

    out = {"n_batches": np.array(n_batches)}
    out.update({"enc_cfg_" + k: np.array(v) for k, v in enc_cfg.items()})
    out.update({"head_cfg_" + k: np.array(v) for k, v in head_cfg.items()})
    out["fusion"] = np.array("concatenation")
    out.update(sd_np(model0, "sd/"))
    out["label_embeddings"], out["label_token_counts"] = lab.numpy(), cnt.numpy()
    for k, b in enumerate(batches):
        out[f"batch{k}/x"], out[f"batch{k}/lens"], out[f"batch{k}/multihots"] = (
            b["sequence_onehots"].numpy(), b["sequence_lengths"].numpy(), b["label_multihots"].numpy())
        out[f"batch{k}/noise_u"] = noises[k].numpy()

    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "parenthood.json"), "w") as f:
        json.dump({}, f)
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "pg"), rank=0, world_size=1)
    real_rand_like = torch.rand_like
    cases = {"adam": ("Adam", True), "adam_frozen_head": ("Adam", False), "adamw": ("AdamW", True),
             "sgd": ("SGD", True), "sgd_frozen_head": ("SGD", False)}
    try:
        for case, (opt_name, train_head) in cases.items():
            params = {"NUM_EPOCHS": 1, "TRAIN_SEQUENCE_ENCODER": False, "LABEL_ENCODER_NUM_TRAINABLE_LAYERS": 0,
                      "TRAIN_PROJECTION_HEAD": train_head, "NORMALIZE_PROBABILITIES": False, "EPOCHS_PER_VALIDATION": 1,
                      "GRADIENT_ACCUMULATION_STEPS": 1, "CLIP_VALUE": 1, "LORA": False, "LABEL_EMBEDDING_DIM": 24,
                      "OPTIMIZER": opt_name, "LEARNING_RATE": 0.003, "WEIGHT_DECAY": 0.01, "DECISION_TH": 0.5,
                      "LOSS_FN": "BCE", "BCE_POS_WEIGHT": 1}
            cfg = {"params": params, "paths": {"PARENTHOOD_LIB_PATH": os.path.join(tmp, "parenthood.json"),
                                               "OUTPUT_MODEL_DIR": os.path.join(tmp, "ckpt")}}
            model = build()
            model.load_state_dict(model0.state_dict())
            loss_fn = get_loss(cfg, bce_pos_weight=torch.tensor(1.0))
            losses, first_logits = [], []

            class _Rec(torch.nn.Module):
                def forward(self, logits, targets):
                    l = loss_fn(logits, targets)
                    losses.append(float(l.detach()))
                    if not first_logits:
                        first_logits.append(logits.detach().numpy().copy())
                    return l

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                trainer = PT.ProtNoteTrainer(model=model, device="cpu", rank=0, config=cfg, logger=logging.getLogger("g"),
                                             timestamp="t", run_name="golden", loss_fn=_Rec(), is_master=False)
                trainer.training_step = 0
                queue = [u.clone() for u in noises]
                PN.torch.rand_like = lambda t, *a, **k: queue.pop(0)
                loader = _Loader(batches)
                loader.dataset = types.SimpleNamespace(label_vocabulary=list(range(n_labels)))
                model.train()
                metrics = trainer.train_one_epoch(loader, _NoMetrics())
            PN.torch.rand_like = real_rand_like
            p = case + "/"
            out[p + "params_json"] = np.array(json.dumps(params))
            out[p + "trainable_names"] = np.array(trainer.trainable_params_names)
            out[p + "optimizer_class"] = np.array(type(trainer.optimizer).__name__)
            out[p + "n_optimizer_params"] = np.array(len(trainer.optimizer.param_groups[0]["params"]))
            out[p + "first_logits"] = first_logits[0]
            out[p + "losses"] = np.array(losses, dtype=np.float64)
            for mk, mv in metrics.items():
                out[p + "metrics/" + mk] = np.array(float(mv))
            out.update(sd_np(model, p + "sd_after/"))
            print(case, type(trainer.optimizer).__name__, len(trainer.trainable_params_names), "trainable,",
                  "losses", [round(v, 5) for v in losses[:3]], "...", metrics)
    finally:
        PN.torch.rand_like = real_rand_like
    np.savez_compressed(os.path.join(OUT, "optimizer_branches.npz"), **out)
    print("optimizer_branches.npz", os.path.getsize(os.path.join(OUT, "optimizer_branches.npz")) // 1024, "KiB")


def golden_disk_formats():
    """On-disk formats either side of the hot path, produced / consumed by the reference's own code:
      * utils/configs.py:74-107 generate_label_embedding_path - the cache-file naming rule, as a table of
        (params, base path) -> path;
      * utils/models.py:304-321 save_checkpoint called on a DistributedDataParallel-wrapped ProtNote (keys carry the
        'module.' prefix, bin/main.py:452) with the Adam the trainer builds, after one optimisation step
        -> tests/golden/disk_formats/ref_checkpoint_ddp.pt, and what utils/models.py:324-374 load_model restores from it;
      * a cached label-embedding pair in the layout bin/generate_label_embeddings.py:93-97,123-164 writes (tensor file +
        `<stem>_index.<ext>` pandas DataFrame with id / description_type / description / token_count), named by
        generate_label_embedding_path, and what the reference's consumer (ProteinDataset, datasets.py:115-127,269-343)
        makes of it: sorted embedding rows and token counts for a vocabulary.  (The producer script itself needs the
        BioGPT download and cannot run here; the pair is written with its last three statements' calls.)"""
    import json
    import logging
    import tempfile

    import pandas as pd
    import torch.distributed as dist
    import Bio.SeqIO as SeqIO

    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.configs import generate_label_embedding_path
    from protnote.utils.models import load_model, save_checkpoint

    out_dir = os.path.join(OUT, "disk_formats")
    os.makedirs(out_dir, exist_ok=True)
    # ---- naming rule ----
    table = []
    for ckpt in ("microsoft/biogpt", "intfloat/e5-large-v2", "intfloat/multilingual-e5-large-instruct"):
        for pool in ("mean", "last_token", "all"):
            for base in ("embeddings/frozen_label_embeddings.pt", "data/embeddings/frozen_label_embeddings_2024.pt",
                         "frozen_ec_embeddings.pt", "a/b/c/go_jul_2024_extra_tag.pkl"):
                params = {"LABEL_ENCODER_CHECKPOINT": ckpt, "LABEL_EMBEDDING_POOLING_METHOD": pool}
                table.append({"params": params, "base": base, "path": generate_label_embedding_path(params, base)})
    bad = None
    try:
        generate_label_embedding_path({"LABEL_ENCODER_CHECKPOINT": "bert-base", "LABEL_EMBEDDING_POOLING_METHOD": "mean"}, "x.pt")
    except AssertionError as e:
        bad = str(e)
    doc = {"naming": table, "unsupported_checkpoint_assertion": bad}

    # ---- checkpoint written by save_checkpoint from a DDP-wrapped model ----
    tmp = tempfile.mkdtemp()
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "pg"), rank=0, world_size=1)
    enc_cfg = dict(num_labels=5, input_channels=20, output_channels=8, kernel_size=9, dilation_base=3,
                   num_resnet_blocks=1, bottleneck_factor=0.5)
    head_cfg = dict(protein_embedding_dim=8, label_embedding_dim=8, latent_dim=4, output_mlp_hidden_dim_scale_factor=2,
                    output_mlp_num_layers=2, projection_head_num_layers=2, projection_head_hidden_dim_scale_factor=2)
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(12)

    def build():
        return ProtNote(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg), label_encoder=None,
                        feature_fusion="concatenation", **head_cfg)

    model = build()
    randomize_(model, g)
    for n, p in model.named_parameters():
        if n.startswith("sequence_encoder"):
            p.requires_grad = False
    ddp = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)
    opt = torch.optim.Adam([p for p in ddp.parameters() if p.requires_grad], lr=1e-3)
    x, _ = onehots(g, [12, 7, 12], 12)
    lens = torch.tensor([12, 7, 12])
    lab = torch.randn(6, 8, generator=g)
    ddp.train()
    logits, _ = ddp(sequence_onehots=x, sequence_lengths=lens, label_embeddings=lab)
    logits.square().mean().backward()
    opt.step()
    ck = os.path.join(out_dir, "ref_checkpoint_ddp.pt")
    save_checkpoint(model=ddp, optimizer=opt, epoch=7, best_val_metric=0.4375, model_path=ck)
    # what the reference's load_model restores from it (into a fresh, unwrapped model + fresh Adam)
    m2 = build()
    for n, p in m2.named_parameters():
        if n.startswith("sequence_encoder"):
            p.requires_grad = False
    tr = types.SimpleNamespace(model=m2, optimizer=torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1.0),
                               starting_epoch=1, epoch=1, best_val_metric=0.0)
    tr._get_model = lambda: m2
    load_model(tr, ck, rank=0, from_checkpoint=True)
    exp = {"ckpt/sd/" + k: v.numpy().copy() for k, v in m2.state_dict().items()}
    osd = tr.optimizer.state_dict()
    for i, st in osd["state"].items():
        exp[f"ckpt/opt/{i}/exp_avg"] = st["exp_avg"].numpy().copy()
        exp[f"ckpt/opt/{i}/exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
        exp[f"ckpt/opt/{i}/step"] = np.array(float(st["step"]))
    doc["checkpoint"] = {"file": "ref_checkpoint_ddp.pt", "epoch": tr.epoch, "starting_epoch": tr.starting_epoch,
                         "best_val_metric": tr.best_val_metric, "optimizer_lr": osd["param_groups"][0]["lr"],
                         "optimizer_param_ids": list(osd["param_groups"][0]["params"]),
                         "enc_cfg": enc_cfg, "head_cfg": head_cfg,
                         "first_key_in_file": list(torch.load(ck, weights_only=False)["model_state_dict"])[0]}

    # ---- cached label-embedding pair, named by the rule, read back by the reference's dataset ----
    params = {"LABEL_ENCODER_CHECKPOINT": "microsoft/biogpt", "LABEL_EMBEDDING_POOLING_METHOD": "mean"}
    rel = generate_label_embedding_path(params, "frozen_label_embeddings.pt")
    out_path = os.path.join(out_dir, rel)
    idx_parts = out_path.split(".")  # generate_label_embeddings.py:93-97 (same rule in datasets.py:115-118)
    idx_path = "_".join([idx_parts[0], "index"]) + "." + idx_parts[1]
    rows = []
    for gid in ["GO:0004", "GO:0001", "GO:0007", "GO:0002", "GO:0003"]:
        for dt, n_d in (("name", 1), ("label", 1), ("synonym_exact", 2)):
            for _ in range(n_d):
                rows.append({"id": gid, "description_type": dt, "description": f"{gid} {dt} {len(rows)}",
                             "token_count": 3 + (5 * len(rows)) % 11})
    embeddings_idx = {k: [r[k] for r in rows] for k in ("id", "description_type", "description", "token_count")}
    embeddings = torch.randn(len(rows), 8, generator=g)
    embeddings_idx = pd.DataFrame(embeddings_idx)
    torch.save(embeddings, out_path)
    torch.save(embeddings_idx, idx_path)

    class _Rec:
        def __init__(self, desc, seq):
            self.description, self.seq = desc, seq

    def _parse(path, fmt):
        desc, seq = None, []
        for line in open(path):
            line = line.rstrip("\n")
            if line.startswith(">"):
                if desc is not None:
                    yield _Rec(desc, "".join(seq))
                desc, seq = line[1:], []
            elif line:
                seq.append(line)
        if desc is not None:
            yield _Rec(desc, "".join(seq))

    SeqIO.parse = _parse
    from protnote.data.datasets import ProteinDataset

    fasta = [("P1", "ACDEFGHIK", ["GO:0002", "GO:0004"]), ("P2", "MKTAYIAK", ["GO:0001"]), ("P3", "GGSGG", ["GO:0003", "GO:0001"])]
    fp = os.path.join(tmp, "toy.fasta")
    with open(fp, "w") as f:
        for sid, seq, labs in fasta:
            f.write(">" + " ".join([sid] + labs) + "\n" + seq + "\n")
    real_load = torch.load
    torch.load = lambda *a, **k: real_load(*a, **{**k, "weights_only": False})
    try:
        cfg = {"params": {"AUGMENT_RESIDUE_PROBABILITY": 0.0, "LABEL_AUGMENTATION_DESCRIPTIONS": "name+label",
                          "TRAIN_SUBSET_FRACTION": 1, "TEST_SUBSET_FRACTION": 1, "VALIDATION_SUBSET_FRACTION": 1,
                          "INFERENCE_GO_DESCRIPTIONS": "name+label", "EXTRACT_VOCABULARIES_FROM": None,
                          "DEDUPLICATE": True, "MAX_SEQUENCE_LENGTH": 100},
               "paths": {}, "LABEL_EMBEDDING_PATH": out_path}
        ds = ProteinDataset({"data_path": fp, "dataset_type": "test"}, cfg, logger=logging.getLogger("g"))
    finally:
        torch.load = real_load
    exp["pair/label_vocabulary"] = np.array(ds.label_vocabulary)
    exp["pair/sorted_label_embeddings"] = ds.sorted_label_embeddings.numpy().copy()
    exp["pair/sorted_label_token_counts"] = np.asarray(ds.sorted_label_token_counts)
    doc["pair"] = {"params": params, "base": "frozen_label_embeddings.pt", "embedding_file": rel,
                   "index_file": os.path.relpath(idx_path, out_dir), "descriptions": ["name", "label"]}
    with open(os.path.join(out_dir, "disk_formats.json"), "w") as f:
        json.dump(doc, f, indent=1)
    np.savez_compressed(os.path.join(out_dir, "expected.npz"), **exp)
    print("disk_formats/", sorted(os.listdir(out_dir)), doc["checkpoint"]["first_key_in_file"], rel)


def golden_grid_samplers():
    """Index streams of protnote/data/samplers.py::GridBatchSampler (Python `random`, seeded) and
    ::GeneralDistributedSampler (rank shards of an arbitrary sampler's stream)."""
    import random

    from protnote.data.samplers import GeneralDistributedSampler, GridBatchSampler

    out = {}
    obs = [5, 3, 8, 0, 9, 1, 7, 2, 6, 4, 10]
    for drop in (False, True):
        for shuf in (True, False):
            random.seed(5)
            s = GridBatchSampler(obs, 4, drop, num_labels=7, labels_batch_size=3, shuffle_grid=shuf)
            for epoch in (0, 1):  # the label permutation carries over between epochs (shuffled in place)
                cells = list(iter(s))
                o = np.full((len(cells), 4), -1, dtype=np.int64)
                l = np.full((len(cells), 3), -1, dtype=np.int64)
                for k, cell in enumerate(cells):
                    ob = [c[0] for c in cell]
                    assert all(c[1] is cell[0][1] or c[1] == cell[0][1] for c in cell)
                    o[k, :len(ob)] = ob
                    l[k, :len(cell[0][1])] = cell[0][1]
                out[f"grid/drop{int(drop)}/shuf{int(shuf)}/e{epoch}/obs"] = o
                out[f"grid/drop{int(drop)}/shuf{int(shuf)}/e{epoch}/labels"] = l
            out[f"grid/drop{int(drop)}/shuf{int(shuf)}/len"] = np.array(len(s))
    stream = [11, 4, 7, 0, 2, 9, 5, 13, 1, 8]
    for drop in (False, True):
        for rank in range(3):
            g = GeneralDistributedSampler(stream, num_replicas=3, rank=rank, drop_last=drop)
            out[f"general/drop{int(drop)}/r{rank}"] = np.array(list(iter(g)))
            out[f"general/drop{int(drop)}/r{rank}/len"] = np.array(len(g))
    np.savez_compressed(os.path.join(OUT, "grid_samplers.npz"), **out)
    print("grid_samplers.npz", len(out))


# --------------------------------------------------------------------------------------------
def golden_config_holes():
    """Two corners of the reference's config surface (VERDICT r04 missing 3-4):
      * OUTPUT_MLP_NUM_LAYERS: 1 (get_mlp, ProtNote.py:337-378: ONE hidden layer + the output neuron) for the three
        concatenation fusions (+ one case without BatchNorm): eval logits (raw / ensembled), eval save_embeddings, one
        train step (BCE) with gradients and post-Adam weights, and the train-mode save_embeddings outputs;
      * save_embeddings=True in TRAIN mode on the 3-layer head (ProtNote.py:292-302,324-332; the trainer passes the flag
        through, ProtNoteTrainer.py:288) and with `similarity` (nothing to save: both lists stay empty)."""
    from protnote.models.protein_encoders import ProteInfer
    from protnote.models.ProtNote import ProtNote
    from protnote.utils.losses import get_loss
    import protnote.models.ProtNote as PN

    enc_cfg = dict(num_labels=7, input_channels=20, output_channels=28, kernel_size=9,
                   dilation_base=3, num_resnet_blocks=2, bottleneck_factor=0.5)
    base = dict(protein_embedding_dim=28, label_embedding_dim=24, latent_dim=16,
                output_mlp_hidden_dim_scale_factor=3, outout_mlp_add_batchnorm=True, projection_head_num_layers=4,
                projection_head_hidden_dim_scale_factor=3, dropout=0.0, label_embedding_noising_alpha=20.0,
                temperature=0.07)
    lens = [50, 3, 21, 50, 17, 44, 9]
    lmax, n_labels = 50, 11
    cases = [("1layer_concatenation", "concatenation", 1, True), ("1layer_concatenation_diff", "concatenation_diff", 1, True),
             ("1layer_concatenation_prod", "concatenation_prod", 1, True), ("1layer_concatenation_nobn", "concatenation", 1, False),
             ("3layer_concatenation", "concatenation", 3, True), ("3layer_concatenation_prod", "concatenation_prod", 3, True),
             ("3layer_similarity", "similarity", 3, True)]
    for name, fusion, nlayers, out_bn in cases:
        head_cfg = dict(base, output_mlp_num_layers=nlayers, outout_mlp_add_batchnorm=out_bn)
        g = torch.Generator().manual_seed(4321)
        torch.manual_seed(3)
        enc = ProteInfer(activation=torch.nn.ReLU, **enc_cfg)
        model = ProtNote(sequence_encoder=enc, label_encoder=None, feature_fusion=fusion,
                         inference_descriptions_per_label=2, **head_cfg)
        randomize_(model, g)
        for n, p in model.named_parameters():
            if n.startswith("sequence_encoder"):
                p.requires_grad = False
        out = {"fusion": np.array(fusion)}
        out.update({"enc_cfg_" + k: np.array(v) for k, v in enc_cfg.items()})
        out.update({"head_cfg_" + k: np.array(v) for k, v in head_cfg.items()})
        out.update(sd_np(model, "sd/"))
        x, _ = onehots(g, lens, lmax)
        lens_t = torch.tensor(lens, dtype=torch.int64)
        lab = torch.randn(n_labels * 2, 24, generator=g)
        counts = torch.randint(3, 30, (n_labels * 2,), generator=g)
        y = (torch.rand(len(lens), n_labels, generator=g) < 0.3).to(torch.int64)
        out.update(x=x.numpy(), lens=lens_t.numpy(), label_embeddings=lab.numpy(),
                   label_token_counts=counts.numpy(), multihots=y.numpy())

        def emb_np(prefix, emb):
            for k in ("output_layer_embeddings", "joint_embeddings"):
                v = emb[k]
                out[prefix + k + "_is_empty_list"] = np.array(isinstance(v, list) and len(v) == 0)
                if not isinstance(v, list):
                    out[prefix + k] = v.numpy().copy()

        model.eval()
        with torch.no_grad():
            lg, emb = model(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab, save_embeddings=True)
            out["eval/logits_ens2"] = lg.numpy()
            emb_np("eval/", emb)
            model.inference_descriptions_per_label = 1
            lg1, _ = model(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab)
            out["eval/logits_raw"] = lg1.numpy()
            model.inference_descriptions_per_label = 2

        lab1 = lab[0::2].contiguous()
        cnt1 = counts[0::2].contiguous()
        u = torch.rand(lab1.shape, generator=g)
        out["train/noise_u"] = u.numpy()
        real_rand_like = torch.rand_like
        PN.torch.rand_like = lambda t, *a, **k: u.clone()
        try:
            m2 = ProtNote(sequence_encoder=ProteInfer(activation=torch.nn.ReLU, **enc_cfg), label_encoder=None,
                          feature_fusion=fusion, inference_descriptions_per_label=2, **head_cfg)
            m2.load_state_dict(model.state_dict())
            for n, p in m2.named_parameters():
                if n.startswith("sequence_encoder"):
                    p.requires_grad = False
            m2.train()
            loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
            from torch.nn.utils import clip_grad_norm_

            params = [p for n, p in m2.named_parameters() if p.requires_grad and not n.startswith("sequence_encoder")]
            opt = torch.optim.Adam(params, lr=3e-4)
            # the train step with save_embeddings=True: the flag does not change the logits or the graph (ProtNote.py:292-302)
            logits, emb = m2(sequence_onehots=x, sequence_lengths=lens_t, label_embeddings=lab1, label_token_counts=cnt1,
                             save_embeddings=True)
            emb_np("train/", emb)
            loss = loss_fn(logits, y.float())
            loss.backward()
            out["train/logits"] = logits.detach().numpy().copy()
            out["train/loss"] = np.array(float(loss.detach()), dtype=np.float32)
            for n, p in m2.named_parameters():
                if p.grad is not None:
                    out["train/grad/" + n] = p.grad.detach().numpy().copy()
            out["train/grad_norm"] = np.array(float(clip_grad_norm_(m2.parameters(), max_norm=1.0)), dtype=np.float32)
            opt.step()
            out.update(sd_np(m2, "train/sd_after/"))
        finally:
            PN.torch.rand_like = real_rand_like
        fn = os.path.join(OUT, f"config_holes_{name}.npz")
        np.savez_compressed(fn, **out)
        print(os.path.basename(fn), os.path.getsize(fn) // 1024, "KiB")


def golden_signatures():
    """inspect.signature of every reference object tests/test_signatures.py holds a twin to: parameter names, kinds and
    default reprs (the test's own NAMES and _sig, so the fixture and the comparison cannot drift apart)."""
    import importlib
    import json

    sys.path.insert(0, os.path.dirname(OUT))
    from test_signatures import NAMES, _sig

    res = {}
    for n in NAMES:
        mod, _, attr = n.partition(":")
        o = importlib.import_module(mod)
        for a in attr.split("."):
            o = getattr(o, a)
        res[n] = _sig(o)
    fn = os.path.join(OUT, "reference_signatures.json")
    with open(fn, "w") as f:  # one object per line
        f.write("{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(res[n])}" for n in sorted(res)) + "\n}\n")
    print(os.path.basename(fn), len(res), "signatures")


def golden_base_config():
    """The reference's configs/base_config.yaml as data: parsed and dumped again (values only, no comments), checked to
    load back to the same mapping."""
    import yaml

    with open(os.path.join(REF, "configs", "base_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    text = yaml.safe_dump(cfg, sort_keys=False)
    assert yaml.safe_load(text) == cfg
    fn = os.path.join(OUT, "base_config.yaml")
    with open(fn, "w") as f:
        f.write(text)
    print(os.path.basename(fn), len(text), "B")


if __name__ == "__main__":
    install_stubs()
    torch.set_num_threads(8)
    only = [a[2:] for a in sys.argv[1:] if a.startswith("--")]
    jobs = {"encoder": golden_encoder, "encoder_pieces": golden_encoder_pieces, "protnote": golden_protnote,
            "protnote_nobn": lambda: golden_protnote([("concatenation", False)]), "losses": golden_losses_metrics, "losses_extra": golden_losses_extra,
            "collator": golden_collator, "bookkeeping": golden_bookkeeping, "tf_weights": golden_tf_weights,
            "samplers": golden_samplers, "attention": golden_attention_pooling, "grid_samplers": golden_grid_samplers,
            "config0": golden_config0_full_width, "optimizer_branches": golden_optimizer_branches,
            "disk_formats": golden_disk_formats, "config_holes": golden_config_holes, "signatures": golden_signatures,
            "base_config": golden_base_config}
    for name, fn in jobs.items():
        if not only or name in only:
            fn()
