"""bench.cpu_baseline — the oracle (`"kind": "port"`) timed on the host cores beside the GPU number (task ④): a bounded sample,
extrapolated; for the Qwen2-Audio workloads it also times one audio-tower layer and the optimizer arithmetic so that the figure
estimates the whole step.  Here: the leg runs on a toy geometry, every term lowers the estimate, the sample says what it was."""
import types

import torch


def _toy(name="qwen2_audio_7b", wav=True):
    class AC:
        d_model, encoder_attention_heads, encoder_ffn_dim, encoder_layers = 64, 4, 128, 2

    class MC:
        audio_config = AC()

    class Cfg:
        hidden_size, intermediate_size, num_attention_heads, num_key_value_heads, head_dim = 64, 128, 4, 4, 16
        vocab_size, rms_norm_eps, rope_theta, rope_scaling, num_hidden_layers = 100, 1e-6, 1e4, None, 2

    return types.SimpleNamespace(seq_cfg=Cfg(), T=2048, B=2, name=name, model_config=MC(),
                                 wav=torch.zeros(3, 10) if wav else None)


def test_cpu_baseline_is_the_oracle_port_and_counts_tower_and_optimizer_for_the_audio_workloads():
    import bench
    threads = torch.get_num_threads()
    try:
        decoder_only = bench.cpu_baseline(_toy(), n_params=0)                  # (no parameter count: decoder + head only)
        whole = bench.cpu_baseline(_toy(), n_params=200_000_000)
        other = bench.cpu_baseline(_toy(name="llama_asr_1b", wav=False), n_params=200_000_000)
    finally:
        torch.set_num_threads(threads)
    for r in (decoder_only, whole, other):
        assert r["kind"] == "port" and r["cores"] >= 1 and r["value"] > 0 and "oracle fp32 eager" in r["sample"]
    assert "Whisper encoder layer" in whole["sample"] and "AdamW" in whole["sample"]
    assert "excluded -> an upper bound" in decoder_only["sample"] and "excluded -> an upper bound" in other["sample"]
    assert whole["value"] < 0.8 * decoder_only["value"]                       # the extra terms cost time


def test_dump_outputs_writes_the_step_statistics_and_a_fixed_sample_of_the_optimizer_state(tmp_path):
    """`bench.py --dump-outputs DIR`: float arrays only, the same positions whatever the values, every position of a
    parameter smaller than the sample, the last step's pipelined updates waited for first."""
    import numpy as np

    import bench

    class Opt:
        waited = 0

        def __init__(self, sizes, seed):
            g = torch.Generator().manual_seed(seed)
            self.state = [dict(master=torch.randn(n, generator=g), m=torch.randn(n, generator=g)) for n in sizes]

        def wait_updates(self):
            Opt.waited += 1

    sizes = [10, bench.DUMP_SAMPLE_PER_TENSOR * 3 + 1, 7]
    stats = {"loss_per_sample": torch.tensor(2.5), "grad_norm": torch.tensor(0.75), "acc": None}
    runs = []
    for seed, d in ((0, tmp_path / "a"), (0, tmp_path / "b"), (1, tmp_path / "c")):
        shapes = bench.dump_outputs(str(d), stats, types.SimpleNamespace(optimizer=Opt(sizes, seed)))
        runs.append({p.stem: np.load(p) for p in d.glob("*.npy")})
        assert set(shapes) == set(runs[-1]) == {"loss_per_sample", "grad_norm", "master_weights_sample", "exp_avg_sample"}
    a, b, c = runs
    assert Opt.waited == 3
    n = 10 + bench.DUMP_SAMPLE_PER_TENSOR + 7
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["master_weights_sample"].shape == a["exp_avg_sample"].shape == (n,)
    assert float(a["loss_per_sample"]) == 2.5 and float(a["grad_norm"]) == 0.75
    assert not np.array_equal(a["master_weights_sample"], c["master_weights_sample"])
    first = Opt(sizes, 0).state[0]["master"].numpy()
    assert np.array_equal(a["master_weights_sample"][:10], first)       # (a small parameter: all of it, in order)
