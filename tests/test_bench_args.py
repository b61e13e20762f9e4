"""bench.py's command line (no GPU): a plain run is the headline alone, `--full` turns the other sections on."""
import sys

import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert (a.full, a.steps, a.warmup, a.workload) == (False, 3, 2, "forward")
    assert _parse(monkeypatch, "--full", "--steps", "3").full


@pytest.mark.parametrize("argv", [("--full", "--forward-only"), ("--inflight", "4")])
def test_full_only_combinations_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_inflight_runs_under_full(monkeypatch):
    assert _parse(monkeypatch, "--full", "--inflight", "4").inflight == 4
    assert _parse(monkeypatch, "--inflight", "0").inflight == 0      # an explicit "off" is no section
