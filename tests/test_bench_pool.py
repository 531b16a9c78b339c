"""The rolling-upgrade benchmark computes the same with and without the
connection pool, and with it the eviction workers reuse connections instead
of dialling one each."""

import os

import numpy as np
import pytest

from k8s_operator_libs_amd.core.restclient import RestClient

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

N_NODES = MAX_PARALLEL = 2
STEPS = 2


def _upgrade(monkeypatch, use_pool):
    monkeypatch.syspath_prepend(REPO)
    import bench

    monkeypatch.setattr(RestClient, "USE_POOL", use_pool)
    stats = []
    real_close = RestClient.close

    def close(self):
        if self._pool is not None:
            stats.append(self._pool.stats())
        real_close(self)

    monkeypatch.setattr(RestClient, "close", close)
    result = bench.run_rolling_upgrade_benchmark(
        n_nodes=N_NODES, steps=STEPS, warmup=0, max_parallel=MAX_PARALLEL,
        collect_outputs=True)
    assert result["upgrades_completed"] == STEPS
    assert len(stats) == 1
    return result["outputs"], stats[0]


@pytest.fixture(scope="module")
def runs():
    mp = pytest.MonkeyPatch()
    try:
        pooled = _upgrade(mp, True)
        local = _upgrade(mp, False)
    finally:
        mp.undo()
    return pooled, local


def test_outputs_are_equal_with_and_without_the_pool(runs):
    (pooled, _), (local, _) = runs
    assert sorted(pooled) == sorted(local) == [
        "driver_pod_on_new_revision", "gpu_validation_max_err",
        "node_final_state", "node_unschedulable", "workload_pods_remaining"]
    for name in pooled:
        assert np.array_equal(pooled[name], local[name]), name
    assert list(pooled["node_final_state"]) == [11.0] * N_NODES
    assert list(pooled["workload_pods_remaining"]) == [0.0] * N_NODES


def test_workers_reuse_connections_instead_of_dialling(runs):
    (_, stats), (_, unused) = runs
    # at any moment the client is used by the reconcile thread and by at most
    # one eviction worker per node of the rolling window; a connection is
    # only dialled when every pooled one is in use, so that many suffice for
    # the whole run, however many worker threads come and go (one per node
    # and step here)
    concurrent_users = 1 + MAX_PARALLEL
    assert stats["dials"] <= concurrent_users
    assert stats["reuses"] > 0
    assert stats["stale_discards"] == 0
    assert unused == {"dials": 0, "reuses": 0, "stale_discards": 0, "idle": 0}
