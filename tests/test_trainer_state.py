"""The trainer's derived device state (captured graphs, workspaces, epoch
buffers, data caches, history) lives in one set of slots that one method
empties; no GPU needed."""
import torch

SLOTS = ("_graphs", "_indexed_ws", "_epoch_bufs", "_pool_cache", "_eval_cache", "_scalars", "_history")


def test_moved_trainer_carries_no_derived_state(tmp_path):
    """Every slot exists right after construction, and .to() / _apply() empties
    all of them (a moved trainer keeps nothing that was built for the old device
    or the old flat parameters); the dropout seed base is not derived state."""
    from heybuddy.trainer import WakeWordTrainer
    tr = WakeWordTrainer(checkpoint_dir=str(tmp_path), device="cpu")
    empty = {s: getattr(tr, s) for s in SLOTS}  # AttributeError here: a slot _init_state does not create
    assert all(v is None or v == {} for v in empty.values())
    for move in (lambda: tr.to("cpu"), lambda: tr._apply(lambda t: t)):
        tr._seed_base_v = 4242
        for s in SLOTS:
            setattr(tr, s, {"sentinel": s} if isinstance(empty[s], dict) else torch.zeros(1))
        move()
        for s in SLOTS:
            got = getattr(tr, s)
            assert (got == {} if isinstance(empty[s], dict) else got is None), s
        assert tr._seed_base_v == 4242 and tr._seed_base == 4242
