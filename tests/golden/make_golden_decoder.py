"""Generates the decoder fixtures by running the reference's own Python on the CPU:

    models/decoders.py       FeatureDecoder (get_encoder's configuration, the normalisation, the module names)   imported as it is
    train_decoder.py         cos_loss imported; the optimiser construction (lines 48-51) extracted with ast and executed

on the office_0 configuration read from the reference's yaml files.  `tinycudann` is stubbed with a CPU module whose `Encoding`
is the float64 restatement of the grid (tests/decoder_reference.py: the definition of `restated()` in
tests/grid_encoding_reference.py) on the f32-cast input, its table initialised exactly as splatloc_amd.grid_encoding.Encoding(seed=
1337) initialises its own, so the table is not stored.  `.cuda()`, open3d and the dataset modules are stubbed as the other
generators stub what this machine lacks.  The MLP is moved to float64 after construction (its initial values are nn.Linear's f32
ones under torch.manual_seed(0)), so every stored result is a float64 one.

Three steps of the reference's loop body (train_decoder.py:69-77) on three fixed batches.  Batch k is made of the first 256 points
of a fixed pool of 320 uniform points (numpy default_rng(100 + k)) for which no hidden pre-activation of the INITIAL reference model
lies within its layer's f32 rounding bar of zero (gamma_K * sum |a w|): an f32 evaluation could switch such a ReLU the other way,
which changes a summed parameter gradient by far more than rounding, and a stored sum cannot have a point taken out afterwards.
About 1.7 % of uniform points are such points (384 hidden units, each within 7e-5 sigma of zero with probability 5.6e-5), so the 1 %
cap on excluded points cannot hold on unfiltered 256-point batches; the filter is applied here, on the reference alone, the pool's
share is stored (`pool_undecided`) and the batches themselves are asserted to have none.  Targets: `decoder_reference.targets(k)`,
rebuilt from a seed by the tests (elementwise numpy, bit-identical everywhere).

Files (data only; nothing of the reference travels), each below 1 MiB:
    decoder.npz        state_dict keys and shapes, config, initial MLP weights, batches, losses, step-1 outputs (f64)
    decoder_grads.npz  step-1 gradients: MLP (f32-rounded f64), table as touched entry indices + values
    decoder_step3.npz  MLP weights after step 3
    decoder_table3.npz the table entries touched by any of the three batches after step 3, as indices + values
Run: python tests/golden/make_golden_decoder.py <path of the reference checkout> (or set SPLATLOC_REFERENCE)."""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
POOL, BATCH = 320, 256


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def reference_config(ref):
    import yaml
    office = yaml.safe_load(open(os.path.join(ref, "configs", "replica_nerf", "office_0.yaml")))
    base = yaml.safe_load(open(os.path.join(ref, office["inherit_from"])))
    return {"scene": office["scene"], "decoder": base["decoder"]}


def optimizer_statements(ref):
    """the two assignments of train_decoder.py:48-51 (trainable_parameters, optimizer)"""
    tree = ast.parse(open(os.path.join(ref, "train_decoder.py")).read())
    body = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
            and n.targets[0].id in ("trainable_parameters", "optimizer")]
    assert [n.targets[0].id for n in body] == ["trainable_parameters", "optimizer"]
    return compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), "train_decoder.py", "exec")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SPLATLOC_REFERENCE"]
    sys.path.insert(0, ref)
    import torch
    from tests import decoder_reference as R
    from tests.golden.make_golden import CudaToCpu

    stub("tinycudann", Encoding=R.RestatedEncoding)
    stub("open3d")
    stub("autoencoder")
    stub("autoencoder.dataset", Autoencoder_dataset=object)
    stub("autoencoder.model", Autoencoder=object)
    stub("utils.dataset", load_dataset=None)
    from models.decoders import FeatureDecoder
    import train_decoder as td
    torch.autograd.set_detect_anomaly(False)      # train_decoder.py:18 switches it on at import

    cfg = reference_config(ref)
    with CudaToCpu():
        torch.manual_seed(0)
        decoder = FeatureDecoder(cfg).cuda()
        out = {"config_bound": np.array(cfg["scene"]["bound"], np.float64), "config_voxel_sdf": np.float64(cfg["scene"]["voxel_sdf"]),
               "config_enc": np.array(cfg["decoder"]["enc"]), "config_hidden_dim": np.int64(cfg["decoder"]["hidden_dim"]),
               "config_num_layers": np.int64(cfg["decoder"]["num_layers"]), "config_final_dim": np.int64(cfg["decoder"]["final_dim"]),
               "resolution_sdf": np.int64(decoder.resolution_sdf)}
        sd = decoder.state_dict()
        out["state_keys"] = np.array(list(sd))
        out["state_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64)
        wkeys = [k for k in sd if k.startswith("feature_net")]
        for i, k in enumerate(wkeys):
            assert sd[k].dtype == torch.float32
            out[f"w0_{i}"] = sd[k].numpy().copy()
        decoder.double()
        lr = 0.001
        ns = {"decoder": decoder, "lr": lr, "torch": torch}
        exec(optimizer_statements(ref), ns)
        optimizer = ns["optimizer"]
        groups = optimizer.param_groups
        out["optimizer_groups"] = np.array([[g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]] for g in groups])

        # the batches: decided points of fixed pools, under the initial model
        ref64 = R.RestatedDecoder(decoder, layout=decoder.encoding.layout)
        lo, hi = out["config_bound"][:, 0], out["config_bound"][:, 1]
        batches, undecided = [], 0
        for k in range(3):
            pool = torch.from_numpy(lo + np.random.default_rng(100 + k).random((POOL, 3)) * (hi - lo))
            keep = ref64.decided(pool)
            undecided += int((~keep).sum())
            b = pool[keep][:BATCH]
            assert b.shape[0] == BATCH and bool(ref64.decided(b).all())       # excluded share of the batch itself: 0 <= 1 %
            batches.append(b)
        out["batches"] = torch.stack(batches).numpy()
        out["pool_undecided"] = np.array([undecided, 3 * POOL], np.int64)
        print("undecided points in the pools: %d of %d" % (undecided, 3 * POOL))

        grads, step3 = {}, {}
        losses, touched = [], []
        table = decoder.encoding.params
        for k in range(3):
            xyz, feat = batches[k], torch.from_numpy(R.targets(k)).cuda()
            outputs = decoder(xyz)
            loss = td.cos_loss(outputs, feat)
            optimizer.zero_grad()
            loss.backward()
            losses.append(float(loss))
            idx = torch.nonzero(table.grad.view(-1, 2).abs().sum(1)).view(-1)
            touched.append(idx)
            if k == 0:
                out["outputs"] = outputs.detach().numpy().copy()
                for i, key in enumerate(wkeys):
                    grads[f"dw_{i}"] = dict(decoder.named_parameters())[key].grad.numpy().astype(np.float32)
                grads["dtable_idx"] = idx.numpy().astype(np.int32)
                grads["dtable_val"] = table.grad.view(-1, 2)[idx].numpy().astype(np.float32)
            optimizer.step()
        out["losses"] = np.array(losses, np.float64)
        idx = torch.unique(torch.cat(touched))
        for i, key in enumerate(wkeys):
            step3[f"w3_{i}"] = dict(decoder.named_parameters())[key].detach().numpy().astype(np.float32)
        table3 = {"table3_idx": idx.numpy().astype(np.int32), "table3_val": table.detach().view(-1, 2)[idx].numpy().astype(np.float32)}
    for name, d in (("decoder.npz", out), ("decoder_grads.npz", grads), ("decoder_step3.npz", step3), ("decoder_table3.npz", table3)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(path, size, "bytes")
        assert size < 1 << 20
    print("losses", losses)


if __name__ == "__main__":
    main()
