"""-m "not gpu": the host side of dVAE training (mem_amd/train_vae.py, mem_amd/vae_train.py): the reference's flags, aliases and
defaults (eventvae/train_vae.py:43-125), the refusals by name, the temperature / learning-rate schedule of train_vae.py:342-353
against a restatement on torch's own ExponentialLR, and the engine's refusal of what the kernels cannot take."""
import math

import pytest
import torch


def test_flags_aliases_and_reference_defaults():
    from mem_amd.train_vae import get_args
    a = get_args(["--data_path", "synthetic"])
    want = dict(output_dir="runs/vae", eval_data_path=None, data_set="npy", timesurface=0, hotpix_num_stds=10, hotpixfilter=1, logtrafo=0,
                gammatrafo=0, gamma=0.5, normalize_events=1, slice_max_evs=30000, max_random_shift_evs=15, rand_aug=1,
                disable_eval=False, dist_eval=False, input_size=224, input_H=128, input_W=128, weights=None, num_workers=4,
                pin_mem=False, save_ckpt_freq=5, resize=False, disable_wandb=False, epochs=20, start_epoch=0, batch_size=8, lr=1e-3,
                lr_decay_rate=0.98, starting_temp=1.0, temp_min=0.5, anneal_rate=1e-6, num_images_save=4, num_tokens=8192,
                num_layers=3, num_resnet_blocks=2, loss="mse", emb_dim=512, hidden_dim=256, kl_loss_weight=0.0, clip=1e-3,
                straight_through=0, distributed_backend=None, deepspeed=None)
    for k, v in want.items():
        assert getattr(a, k) == v, (k, getattr(a, k), v)
    b = get_args(["--data_path", "x", "--vae_epochs", "3", "--vae_batch_size", "16", "--vae_lr", "2e-4", "--vae_lr_decay", "0.9",
                  "--vae_num_resnet_blocks", "1", "--vae_loss", "cosine", "--vae_hidden_dim", "128", "--vae_kl_loss_weight", "0.5",
                  "--vae_grad_clip", "0.1", "--vae_straight_through", "1", "--vae_save_ckpt_freq", "2", "--some_other_stage_flag", "7"])
    assert (b.epochs, b.batch_size, b.lr, b.lr_decay_rate, b.num_resnet_blocks, b.loss, b.hidden_dim, b.kl_loss_weight, b.clip,
            b.straight_through, b.save_ckpt_freq) == (3, 16, 2e-4, 0.9, 1, "cosine", 128, 0.5, 0.1, 1, 2)
    with pytest.raises(SystemExit):
        get_args([])                                         # --data_path is required, as in the reference


def test_refused_flags_name_themselves():
    from mem_amd.train_vae import get_args, refuse
    refuse(get_args(["--data_path", "synthetic", "--disable_wandb"]), environ={})
    for argv, name in ((["--distributed_backend", "horovod"], "--distributed_backend"), (["--distr_backend", "deepspeed"], "--distr_backend"),
                       (["--deepspeed"], "--deepspeed"), (["--deepspeed", "1"], "--deepspeed")):
        with pytest.raises(SystemExit) as e:
            refuse(get_args(["--data_path", "synthetic"] + argv), environ={})
        assert name in str(e.value) and "single-GPU" in str(e.value), str(e.value)
    with pytest.raises(SystemExit) as e:
        refuse(get_args(["--data_path", "synthetic"]), environ={"WORLD_SIZE": "2"})
    assert "WORLD_SIZE=2" in str(e.value) and "single-GPU" in str(e.value)
    refuse(get_args(["--data_path", "synthetic"]), environ={"WORLD_SIZE": "1"})


def test_schedule_is_the_reference_loop_bit_for_bit():
    """20 001 iterations of one epoch, then the first of the next: temp and lr before every step equal a restatement of
    train_vae.py:342-353 that uses torch.optim.lr_scheduler.ExponentialLR itself."""
    from mem_amd.train_vae import Schedule, get_args
    args = get_args(["--data_path", "synthetic", "--anneal_rate", "3e-5", "--lr", "1e-3", "--lr_decay_rate", "0.98", "--temp_min", "0.5"])
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=args.lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(optimizer=opt, gamma=args.lr_decay_rate)
    temp, global_step = args.starting_temp, 0
    mine = Schedule(args)
    changes = 0
    for epoch_len in (20001, 1):
        for i in range(epoch_len):
            assert mine.temp == temp and mine.lr == sched.get_last_lr()[0], (i, mine.temp, temp, mine.lr, sched.get_last_lr()[0])
            if i % 10000 == 0:                               # train_vae.py:342-353
                temp = max(temp * math.exp(-args.anneal_rate * global_step), args.temp_min)
                opt.step()
                sched.step()
                changes += 1
            global_step += 1
            mine.after_step(i)
    assert mine.global_step == 20002 and changes == 4
    assert mine.temp == temp and mine.lr == sched.get_last_lr()[0] and mine.temp < args.starting_temp and mine.lr < args.lr


def test_engine_refuses_by_name():
    from mem_amd.vae_model import DiscreteVAE
    from mem_amd.vae_train import DVAEEngine
    cfg = dict(input_H=32, input_W=32, num_tokens=128, codebook_dim=32, num_layers=2, num_resnet_blocks=1, hidden_dim=64)
    for bad, name in ((dict(hidden_dim=96), "hidden_dim=96"), (dict(channels=5), "channels=5"), (dict(num_tokens=100), "num_tokens=100")):
        with pytest.raises(ValueError) as e:
            DVAEEngine(DiscreteVAE(**dict(cfg, **bad)))
        assert name in str(e.value), str(e.value)


def test_discrete_vae_forward_points_at_the_engine():
    from mem_amd.vae_model import DiscreteVAE
    m = DiscreteVAE(input_H=16, input_W=16, num_tokens=16, codebook_dim=8, num_layers=2, hidden_dim=8)
    with pytest.raises(NotImplementedError) as e:
        m(torch.zeros(1, 3, 16, 16))
    assert "DVAEEngine" in str(e.value) and "train_vae" in str(e.value)


def test_config_file_sets_values_and_explicit_flags_win(tmp_path):
    """--config FILE (train_vae.py:43-47): `key = value` lines with the pipeline's vae_* keys set the values; flags on the
    command line win; keys of other stages are ignored."""
    from mem_amd.train_vae import get_args
    cfg = tmp_path / "pipeline.conf"
    cfg.write_text("# shared by the three stages\ndata_path = synthetic\nvae_epochs = 7\nvae_batch_size = 32\nvae_lr = 3e-4  # comment\n"
                   "vae_hidden_dim = 384\nvae_num_resnet_blocks = 3\nvae_loss = smooth_l1\nvae_kl_loss_weight = 0.25\nvae_grad_clip = 0.5\n"
                   "vae_straight_through = 1\ninput_H = 224\ninput_W = 224\nnum_layers = 4\npt_epochs = 300\nexpname =\n")
    a = get_args(["--config", str(cfg)])
    assert (a.data_path, a.epochs, a.batch_size, a.lr, a.hidden_dim, a.num_resnet_blocks, a.loss, a.kl_loss_weight, a.clip,
            a.straight_through, a.input_H, a.input_W, a.num_layers) == ("synthetic", 7, 32, 3e-4, 384, 3, "smooth_l1", 0.25, 0.5, 1, 224, 224, 4)
    assert a.expname == "test" and a.num_tokens == 8192            # an empty value and an absent key keep the defaults
    b = get_args(["--vae_batch_size", "4", "--config", str(cfg), "--hidden_dim", "128", "--epochs", "2"])
    assert (b.batch_size, b.hidden_dim, b.epochs, b.lr, b.num_layers) == (4, 128, 2, 3e-4, 4)
