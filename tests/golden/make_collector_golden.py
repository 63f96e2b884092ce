"""Generate tests/golden/collector_episodes.pt by EXECUTING THE REFERENCE'S COLLECTOR (build container only).

    python tests/golden/make_collector_golden.py

Imports /root/reference/src (with the stubs of `_refimport.py`) and runs the reference's own make_collector, make_env_loop, Dataset
and Episode on the scripted env and policy of tests/collector_cases.py, with num_envs 1 and 3: three NumToCollect(steps=...) on a
train collector (episodes grow across the collects), Dataset.clear(), two NumToCollect(episodes=...) with reset_every_collect.
The file holds data only: per collect the logs and the dataset's lengths, start_idx and counts; after each of the two phases the
dataset's episodes as uint8 levels.  tests/test_collector_simt.py and tests/test_gpu_collector.py hold diamond_amd.collector
against it.
"""
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refimport as R  # noqa: E402

R.install()

from tests import collector_cases as CC  # noqa: E402


def snapshot(ds):
    return {"num_episodes": int(ds.num_episodes), "num_steps": int(ds.num_steps), "lengths": ds.lengths.tolist(), "start_idx": ds.start_idx.tolist(),
            "counts_rew": list(ds.counts_rew), "counts_end": list(ds.counts_end)}


def episodes_u8(ds):
    """The dataset's episodes back to back (split them by `lengths`); `final_row[i]` is episode i's row of `finals`, or -1."""
    eps, finals, final_row = [], [], []
    for i in range(ds.num_episodes):
        e = ds.load_episode(i)
        final = e.info.get("final_observation")
        assert torch.equal(CC.dequant(CC.levels(e.obs)), e.obs) and e.end.dtype == e.trunc.dtype == torch.uint8
        assert final is None or (final.shape == CC.FRAME and torch.equal(CC.dequant(CC.levels(final)), final))
        eps.append(e)
        final_row.append(-1 if final is None else len(finals))
        if final is not None:
            finals.append(CC.levels(final))
    out = {k: torch.cat([getattr(e, k) for e in eps]) for k in ("act", "rew", "end", "trunc")}
    out.update(obs=CC.levels(torch.cat([e.obs for e in eps])), lengths=[len(e) for e in eps], final_row=final_row,
               finals=torch.stack(finals) if finals else torch.zeros((0,) + CC.FRAME, dtype=torch.uint8))
    return out


def main():
    from coroutines.collector import NumToCollect, make_collector
    from data import Dataset

    out = {}
    for num_envs in CC.NUM_ENVS:
        with tempfile.TemporaryDirectory() as tmp:
            ds = Dataset(os.path.join(tmp, CC.NAME), CC.NAME, cache_in_ram=True, save_on_disk=False)
            collects, phases = [], {}
            for i, logs in enumerate(CC.run_script(num_envs, make_collector, NumToCollect, ds)):
                collects.append({"logs": logs, "dataset": snapshot(ds)})
                if i in (2, 4):
                    phases["train" if i == 2 else "test"] = episodes_u8(ds)
        out[num_envs] = {"collects": collects, "episodes": phases}
        # what the script is meant to exercise
        train = phases["train"]
        grown = [c["dataset"]["lengths"] for c in collects[:3]]
        assert any(a != b for g0, g1 in zip(grown, grown[1:]) for a, b in zip(g0, g1)), "no episode grew across two collects"
        assert int(train["end"].sum()) and int(train["trunc"].sum()) and -1 in train["final_row"] and max(train["final_row"]) >= 0
        assert all(len(c["logs"]) >= 1 for c in collects) and sum(len(c["logs"]) for c in collects) > 10
        assert [len(c["logs"]) - 1 >= n for c, n in zip(collects[3:], CC.TEST_EPISODES)] == [True, True]
    path = os.path.join(HERE, "collector_episodes.pt")
    torch.save(out, path)
    print(f"wrote collector_episodes.pt: {os.path.getsize(path) / 1024:.1f} KiB")
    for n, o in out.items():
        print(n, [c["dataset"]["lengths"] for c in o["collects"]])


if __name__ == "__main__":
    main()
