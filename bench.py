#!/usr/bin/env python3
"""Flagship benchmark: 8-node rolling amdgpu-driver upgrade (BASELINE config #3).

Measures the metric BASELINE.json names — rolling-upgrade wall-clock and
reconcile p50 for an 8-node amdgpu driver bump with maxParallelUpgrades=2,
cordon+drain of synthetic ``amd.com/gpu`` pods.  The reference publishes no
numbers, so these runs establish the baseline.

The HEADLINE substrate is the production-shaped stack: state machine ->
CachedClient (watch-fed informers) -> RestClient -> HTTP apiserver
(``--substrate cached``, the default).  ``--substrate http`` drops the
informer cache (direct REST), ``--substrate inproc`` is the round-1
in-process dict store, kept for continuity.  A plain run measures only the
selected substrate; ``--full`` adds comparison runs of the other two
(reduced step count) to the same JSON line.

One *step* = one complete rolling upgrade of an 8-node cluster: every node
travels upgrade-required -> cordon -> wait-for-jobs -> pod-deletion -> drain
-> driver-pod-restart -> validate -> uncordon -> done, driven by repeated
build_state/apply_state reconcile ticks.  With a GPU present, each node's
validation step actually executes the native gfx950 health-check kernels
(MFMA matrix-core smoke) on this rank's device, so the number is grounded in
real MI355X validation work; without a GPU the validator pod is marked ready
directly (CPU-only mode, reported in the JSON).

Scaling is weak: each rank runs an independent 8-node cluster upgrade
(one rank per GPU over torch.distributed, rendezvous provided by the driver).

Flags beyond the driver contract (--gpus/--steps/--warmup):
  --nodes N        simulated cluster size per rank (default 8)
  --max-parallel   rolling window (default 2, the BASELINE config)
  --substrate      cached (default, headline) | http | inproc
  --mode           inplace (default) | requestor (maintenance-operator
                   delegation) | anic (BASELINE config #4: NIC/xGMI driver,
                   wait-for-jobs + xGMI-fabric validation hooks)
  --no-converge    strict reference semantics (one transition per tick)
  --no-gpu-validate  skip the native MFMA/xGMI checks in the validation step
  --full           also run the comparison measurements (the two
                   non-headline substrates); off by default
  --dump-outputs DIR  write what the last timed step computed as
                   DIR/<name>.npy (see collect_step_outputs)
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import time

from k8s_operator_libs_amd.api.upgrade.v1alpha1 import DriverUpgradePolicySpec
from k8s_operator_libs_amd.core import FakeClient
from k8s_operator_libs_amd.core.errors import NotFoundError
from k8s_operator_libs_amd.upgrade import consts, util
from k8s_operator_libs_amd.upgrade.drain import gpu_pod_deletion_filter
from k8s_operator_libs_amd.upgrade.pod_manager import StaleClusterViewError
from k8s_operator_libs_amd.upgrade.state_manager import (
    BuildStateError,
    ClusterUpgradeStateManager,
)

DRIVER_NS = "amd-gpu-operator"
VALIDATOR_SELECTOR = "app=amd-gpu-validator"
COMM_JOB_SELECTOR = "app=comm-job"


def _driver_labels(mode: str) -> dict:
    name = "anic" if mode == "anic" else "amdgpu"
    return {"app": f"{name}-driver-daemonset"}


def _driver_ds_name(mode: str) -> str:
    return "anic-driver" if mode == "anic" else "amdgpu-driver"


# default (amdgpu in-place) labels, importable by the example operator
DRIVER_LABELS = _driver_labels("inplace")


# ---------------------------------------------------------------------------
# synthetic cluster construction
# ---------------------------------------------------------------------------

def _make_cluster(sim, n_nodes, old_hash, new_hash, gpu_pods_per_node=2,
                  mode="inplace"):
    """Create the synthetic driver cluster directly in the backing store
    (cluster-side setup, the envtest Status().Update pattern); the library
    itself talks to it through whichever substrate is under test.  Returns
    (ds, cleanup) where cleanup removes every object this call created."""
    labels = _driver_labels(mode)
    ds_name = _driver_ds_name(mode)
    created = []  # (api_version, kind, name, namespace)

    def mk(obj):
        out = sim.create(obj)
        created.append((obj["apiVersion"], obj["kind"],
                        out["metadata"]["name"],
                        out["metadata"].get("namespace", "")))
        return out

    ds = mk({
        "apiVersion": "apps/v1", "kind": "DaemonSet",
        "metadata": {"name": ds_name, "namespace": DRIVER_NS,
                     "labels": labels},
        "spec": {"selector": {"matchLabels": labels},
                 "template": {"metadata": {"labels": labels}}},
        "status": {"desiredNumberScheduled": n_nodes},
    })
    for rev, h in ((1, old_hash), (2, new_hash)):
        mk({
            "apiVersion": "apps/v1", "kind": "ControllerRevision",
            "metadata": {"name": f"{ds_name}-{h}", "namespace": DRIVER_NS,
                         "labels": dict(labels)},
            "revision": rev,
        })
    for i in range(n_nodes):
        node = f"mi355x-{i}"
        mk({
            "apiVersion": "v1", "kind": "Node",
            "metadata": {"name": node, "labels": {}, "annotations": {}},
            "spec": {},
            "status": {"conditions": [{"type": "Ready", "status": "True"}],
                       "capacity": {"amd.com/gpu": "8"}},
        })
        pod_labels = dict(labels)
        pod_labels["controller-revision-hash"] = old_hash
        mk({
            "apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": f"{ds_name}-{node}", "namespace": DRIVER_NS,
                         "labels": pod_labels,
                         "ownerReferences": [{"apiVersion": "apps/v1",
                                              "kind": "DaemonSet",
                                              "name": ds_name,
                                              "uid": ds["metadata"]["uid"],
                                              "controller": True}]},
            "spec": {"nodeName": node,
                     "containers": [{"name": "driver", "image": f"{ds_name}:old"}]},
            "status": {"phase": "Running",
                       "containerStatuses": [{"name": "driver", "ready": True,
                                              "restartCount": 0}]},
        })
        # synthetic GPU workload pods that must be evicted before the bump
        for j in range(gpu_pods_per_node):
            mk({
                "apiVersion": "v1", "kind": "Pod",
                "metadata": {"name": f"train-{node}-{j}", "namespace": "default",
                             "labels": {"app": "training"},
                             "ownerReferences": [{"apiVersion": "apps/v1",
                                                  "kind": "ReplicaSet",
                                                  "name": "train-rs",
                                                  "uid": f"rs-uid-{i}-{j}",
                                                  "controller": True}]},
                "spec": {"nodeName": node,
                         "containers": [{"name": "t", "image": "train",
                                         "resources": {"limits": {"amd.com/gpu": "8"}}}]},
                "status": {"phase": "Running",
                           "containerStatuses": [{"name": "t", "ready": True,
                                                  "restartCount": 0}]},
            })
        if mode == "anic":
            # in-flight collective-communication jobs the NIC upgrade must
            # wait out (BASELINE config #4's wait-for-jobs hook)
            mk({
                "apiVersion": "v1", "kind": "Pod",
                "metadata": {"name": f"comm-{node}", "namespace": "default",
                             "labels": {"app": "comm-job"}},
                "spec": {"nodeName": node,
                         "containers": [{"name": "allreduce", "image": "rccl-job"}]},
                "status": {"phase": "Running",
                           "containerStatuses": [{"name": "allreduce",
                                                  "ready": True,
                                                  "restartCount": 0}]},
            })
        # validation pod (not ready until the GPU health check passes)
        mk({
            "apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": f"validator-{node}", "namespace": DRIVER_NS,
                         "labels": {"app": "amd-gpu-validator"}},
            "spec": {"nodeName": node,
                     "containers": [{"name": "v", "image": "amd-gpu-validator"}]},
            "status": {"phase": "Running",
                       "containerStatuses": [{"name": "v", "ready": False,
                                              "restartCount": 0}]},
        })

    def cleanup():
        # driver pods may have been recreated under the same name; workload
        # pods may already be evicted — delete whatever still exists
        for api_version, kind, name, ns in reversed(created):
            try:
                sim.delete(api_version, kind, name, ns)
            except Exception:
                pass

    return ds, cleanup


class _DsController:
    """Recreates deleted driver pods with the new revision (the DaemonSet
    controller + kubelet role, like envtest tests do by hand).  Installed
    once per substrate; ``retarget`` points it at each iteration's
    DaemonSet."""

    def __init__(self, cluster, ds, new_hash, labels):
        import threading

        self.cluster, self.ds, self.new_hash = cluster, ds, new_hash
        self.labels = labels
        self._lock = threading.Lock()
        cluster.add_change_hook(self._on_change)

    def retarget(self, ds):
        with self._lock:
            self.ds = ds

    def _on_change(self, event_type, obj):
        if event_type != "DELETED" or obj.get("kind") != "Pod":
            return
        with self._lock:
            refs = obj.get("metadata", {}).get("ownerReferences") or []
            if not refs or refs[0].get("uid") != self.ds["metadata"]["uid"]:
                return
            labels = dict(self.labels)
            labels["controller-revision-hash"] = self.new_hash
            self.cluster.create({
                "apiVersion": "v1", "kind": "Pod",
                "metadata": {"name": obj["metadata"]["name"],
                             "namespace": obj["metadata"]["namespace"],
                             "labels": labels,
                             "ownerReferences": refs},
                "spec": {"nodeName": obj["spec"].get("nodeName", ""),
                         "containers": [{"name": "driver", "image": "driver:new"}]},
                "status": {"phase": "Running",
                           "containerStatuses": [{"name": "driver", "ready": True,
                                                  "restartCount": 0}]},
            })


class _MaintenanceOperatorSim:
    """Minimal maintenance operator for requestor-mode benchmarking: drives
    NodeMaintenance objects to Ready (cordon + evict) and honours deletion
    via a finalizer (uncordon on release)."""

    FINALIZER = "maintenance.amd.com/guard"

    def __init__(self, cluster):
        import threading

        self.cluster = cluster
        self._lock = threading.RLock()
        cluster.add_change_hook(self._on_change)

    def _on_change(self, event_type, obj):
        if obj.get("kind") != "NodeMaintenance" or event_type not in ("ADDED", "MODIFIED"):
            return
        with self._lock:
            api = "maintenance.amd.com/v1alpha1"
            try:
                live = self.cluster.get(api, "NodeMaintenance",
                                        obj["metadata"]["name"],
                                        obj["metadata"].get("namespace", ""))
            except Exception:
                return
            node = live.get("spec", {}).get("nodeName", "")
            if "deletionTimestamp" in live["metadata"]:
                if node:
                    self.cluster.patch("v1", "Node", node,
                                       {"spec": {"unschedulable": None}})
                self.cluster.patch(api, "NodeMaintenance", live["metadata"]["name"],
                                   {"metadata": {"finalizers": []}},
                                   live["metadata"].get("namespace", ""))
                return
            fins = live["metadata"].get("finalizers") or []
            if self.FINALIZER not in fins:
                self.cluster.patch(api, "NodeMaintenance", live["metadata"]["name"],
                                   {"metadata": {"finalizers": fins + [self.FINALIZER]}},
                                   live["metadata"].get("namespace", ""))
            conds = live.get("status", {}).get("conditions") or []
            if not any(c.get("type") == "Ready" for c in conds):
                if node:
                    self.cluster.patch("v1", "Node", node,
                                       {"spec": {"unschedulable": True}})
                    for pod in self.cluster.list("v1", "Pod",
                                                 field_selector=f"spec.nodeName={node}"):
                        refs = pod["metadata"].get("ownerReferences") or []
                        if refs and refs[0].get("kind") == "DaemonSet":
                            continue
                        if pod["metadata"].get("labels", {}).get("app") == "amd-gpu-validator":
                            continue
                        try:
                            self.cluster.delete("v1", "Pod", pod["metadata"]["name"],
                                                pod["metadata"].get("namespace", ""))
                        except Exception:
                            pass
                self.cluster.patch(api, "NodeMaintenance", live["metadata"]["name"],
                                   {"status": {"conditions": [
                                       {"type": "Ready", "status": "True",
                                        "reason": "Ready"}]}},
                                   live["metadata"].get("namespace", ""))


def _run_gpu_validation(device, mode="inplace"):
    """The validation-pod payload on this rank's GPU.  Raises if the native
    extension is missing on a GPU box.

    - amdgpu modes: native gfx950 MFMA matrix-core smoke.
    - anic mode (NIC/xGMI driver, BASELINE config #4): probe the xGMI
      fabric — peer reachability + per-link p2p bandwidth
      (native/gpu_validator.hip xgmi_p2p_probe); on a single-GPU box there
      are no peers, so fall back to the MFMA smoke (still real GPU work)
      and note it.
    """
    from k8s_operator_libs_amd.validation import load_native_validator

    native = load_native_validator()
    if native is None:
        raise RuntimeError("GPU validation requested but native validator missing")
    if mode == "anic":
        links = native.xgmi_p2p_probe(device, 64.0, 2)
        if links:
            bad = [l for l in links if not l.get("accessible") or "error" in l]
            if bad:
                raise RuntimeError(f"xGMI validation failed: {bad}")
            return min(l.get("bandwidth_gbps", 0.0) for l in links)
    err = native.mfma_f32_check(device)
    if err > 1e-6:
        raise RuntimeError(f"MFMA validation failed: err={err}")
    bf16_err = native.mfma_bf16_check(device)
    if bf16_err > 5e-2:
        raise RuntimeError(f"bf16 MFMA validation failed: err={bf16_err}")
    return max(err, bf16_err)


# upgrade-state label values in lifecycle order; a node's final state is
# dumped as its index here (so "upgrade-done" is 11.0)
_STATE_ORDER = (
    consts.UPGRADE_STATE_UNKNOWN,
    consts.UPGRADE_STATE_UPGRADE_REQUIRED,
    consts.UPGRADE_STATE_CORDON_REQUIRED,
    consts.UPGRADE_STATE_WAIT_FOR_JOBS_REQUIRED,
    consts.UPGRADE_STATE_POD_DELETION_REQUIRED,
    consts.UPGRADE_STATE_DRAIN_REQUIRED,
    consts.UPGRADE_STATE_NODE_MAINTENANCE_REQUIRED,
    consts.UPGRADE_STATE_POST_MAINTENANCE_REQUIRED,
    consts.UPGRADE_STATE_POD_RESTART_REQUIRED,
    consts.UPGRADE_STATE_VALIDATION_REQUIRED,
    consts.UPGRADE_STATE_UNCORDON_REQUIRED,
    consts.UPGRADE_STATE_DONE,
    consts.UPGRADE_STATE_FAILED,
)


def collect_step_outputs(sim, n_nodes, state_key, new_hash, validation_errs):
    """What one finished rolling-upgrade step computed, as float64 arrays
    indexed by node (``mi355x-0`` .. ``mi355x-<n-1>``), read from the
    authoritative store before the step's cluster is torn down.

    - ``node_final_state`` [n]: index of the node's upgrade-state label in
      ``_STATE_ORDER`` (-1 if the label holds something else)
    - ``node_unschedulable`` [n]: 1.0 if the node is still cordoned
    - ``driver_pod_on_new_revision`` [n]: 1.0 if the node's driver pod
      carries the new controller-revision hash
    - ``workload_pods_remaining`` [n]: GPU workload pods left on the node
    - ``gpu_validation_max_err`` [n]: the figure the node's native GPU
      validation returned (max abs error of the MFMA f32/bf16 tiles vs the
      CPU reference, or the slowest xGMI link's GB/s when the anic probe
      found peers); -1.0 where no GPU validation ran

    The cluster and the kernels' operands are fixed, so two runs with the
    same arguments produce identical inputs and comparable outputs.
    """
    import numpy as np

    names = [f"mi355x-{i}" for i in range(n_nodes)]
    nodes = {n["metadata"]["name"]: n for n in sim.list("v1", "Node")}
    pods = sim.list("v1", "Pod")
    out = {k: np.zeros(n_nodes, dtype=np.float64) for k in (
        "node_final_state", "node_unschedulable",
        "driver_pod_on_new_revision", "workload_pods_remaining",
        "gpu_validation_max_err")}
    for i, name in enumerate(names):
        node = nodes.get(name, {"metadata": {}})
        label = (node["metadata"].get("labels") or {}).get(state_key, "")
        out["node_final_state"][i] = (
            _STATE_ORDER.index(label) if label in _STATE_ORDER else -1)
        out["node_unschedulable"][i] = float(
            bool((node.get("spec") or {}).get("unschedulable")))
        on_node = [p for p in pods
                   if (p.get("spec") or {}).get("nodeName") == name]
        out["driver_pod_on_new_revision"][i] = float(any(
            (p["metadata"].get("labels") or {}).get(
                "controller-revision-hash") == new_hash for p in on_node))
        out["workload_pods_remaining"][i] = sum(
            1 for p in on_node
            if (p["metadata"].get("labels") or {}).get("app") == "training")
        out["gpu_validation_max_err"][i] = validation_errs.get(name, -1.0)
    return out


def _build_substrate(substrate):
    """Returns (client, sim_cluster, close_fn) for the requested substrate.

    - ``inproc``: direct dict-backed FakeClient (round-1 continuity number)
    - ``http``:   RestClient -> HTTP apiserver (wire-level, no cache)
    - ``cached``: CachedClient informers -> RestClient -> HTTP apiserver
                  (the production architecture; HEADLINE)
    """
    if substrate == "inproc":
        client = FakeClient()
        return client, client.cluster, lambda: None
    from k8s_operator_libs_amd.core.apiserver import start_apiserver
    from k8s_operator_libs_amd.core.restclient import RestClient

    handle = start_apiserver()
    rest = RestClient(handle.url)
    if substrate == "http":
        def close():
            rest.close()
            handle.stop()
        return rest, handle.cluster, close
    if substrate == "cached":
        from k8s_operator_libs_amd.core.cache import CachedClient

        cached = CachedClient(rest)

        def close():
            cached.stop()
            rest.close()
            handle.stop()
        return cached, handle.cluster, close
    raise ValueError(f"unknown substrate {substrate!r}")


def run_rolling_upgrade_benchmark(
    n_nodes=8, steps=10, warmup=2, max_parallel=2, gpu_validate=False,
    device=0, gpu_pods_per_node=2, converge=True,
    mode="inplace", substrate="cached", collect_outputs=False,
):
    """Run `warmup` untimed + `steps` timed full rolling upgrades; returns a
    result dict (single-process path; bench main() adds distribution).

    ``converge=True`` uses the manager's converging reconcile (nodes travel
    every synchronously-completable transition per call); ``False`` uses the
    reference's one-transition-per-tick semantics.  ``collect_outputs=True``
    adds ``outputs`` (see collect_step_outputs) for the last timed step.
    """
    from k8s_operator_libs_amd.metrics import MetricsRegistry
    from k8s_operator_libs_amd.upgrade.requestor import RequestorOptions
    from k8s_operator_libs_amd.upgrade.state_manager import StateOptions

    policy_doc = {
        "autoUpgrade": True,
        "maxParallelUpgrades": max_parallel,
        "maxUnavailable": "50%",
        "podDeletion": {"force": False, "deleteEmptyDir": True},
        "drain": {"enable": True, "timeoutSeconds": 300},
    }
    if mode == "anic":
        # BASELINE config #4: NIC upgrades wait out in-flight communication
        # jobs before quiescing the node (docs/automatic-ofed-upgrade.md)
        policy_doc["waitForCompletion"] = {
            "podSelector": COMM_JOB_SELECTOR, "timeoutSeconds": 300,
        }
    policy = DriverUpgradePolicySpec.model_validate(policy_doc)

    prev_driver = util.get_driver_name()
    util.set_driver_name("anic" if mode == "anic" else "amdgpu")
    state_key = util.get_upgrade_state_label_key()
    driver_labels = _driver_labels(mode)

    wall_times = []
    tick_times = []
    ticks_per_upgrade = []
    completed = 0
    outputs = None

    client, sim, close_substrate = _build_substrate(substrate)
    # in-process ops are microseconds: per-node fan-out is pure overhead
    # there (it pays off when each op is an HTTP round trip); saved and
    # restored so secondary-substrate runs in the same process are unaffected
    from k8s_operator_libs_amd.upgrade.common_manager import CommonUpgradeManager

    prev_fanout = CommonUpgradeManager.MAX_PARALLEL_NODE_OPS
    if substrate == "inproc":
        CommonUpgradeManager.MAX_PARALLEL_NODE_OPS = 1
    ctrl = _DsController(sim, {"metadata": {"uid": "-"}}, "newrev", driver_labels)
    if mode == "requestor":
        _MaintenanceOperatorSim(sim)

    try:
        for it in range(warmup + steps):
            timed = it >= warmup
            ds, cleanup = _make_cluster(sim, n_nodes, "oldrev", "newrev",
                                        gpu_pods_per_node, mode=mode)
            ctrl.retarget(ds)
            # eventually-consistent substrates: wait until the client view
            # reflects the fully-built cluster before the timed region (the
            # production analogue is controller-runtime WaitForCacheSync)
            # the client must see the COMPLETE object set before the timed
            # region: a partial view (e.g. train pods not yet cached) makes
            # the eviction count mismatch and costs extra state hops
            want_default_ns = n_nodes * gpu_pods_per_node + (
                n_nodes if mode == "anic" else 0)
            deadline = time.monotonic() + 30
            while time.monotonic() < deadline:
                try:
                    dss = client.list_daemonsets(namespace=DRIVER_NS,
                                                 label_selector=",".join(
                                                     f"{k}={v}" for k, v in
                                                     driver_labels.items()))
                    driver_ns_pods = client.list_pods(namespace=DRIVER_NS)
                    n_driver = len([p for p in driver_ns_pods
                                    if p["metadata"]["labels"].get(
                                        "controller-revision-hash")])
                    n_validator = len([p for p in driver_ns_pods
                                       if p["metadata"]["labels"].get("app")
                                       == "amd-gpu-validator"])
                    n_workload = len(client.list_pods(namespace="default"))
                    n_revs = len(client.list_controller_revisions(
                        namespace=DRIVER_NS))
                    if (dss and n_revs >= 2 and n_driver >= n_nodes
                            and n_validator >= n_nodes
                            and n_workload >= want_default_ns
                            and len(client.list_nodes()) >= n_nodes):
                        break
                except Exception:
                    pass
                time.sleep(0.001)
            registry = MetricsRegistry()
            options = None
            if mode == "requestor":
                options = StateOptions(requestor=RequestorOptions(
                    use_maintenance_operator=True,
                    requestor_id="amd.gpu.operator",
                    namespace="default",
                ))
            manager = (
                ClusterUpgradeStateManager(client, metrics=registry,
                                           options=options)
                .with_pod_deletion_enabled(gpu_pod_deletion_filter)
                .with_validation_enabled(VALIDATOR_SELECTOR)
            )
            validation_errs = {}
            t0 = time.perf_counter()
            rounds = 0
            last_done = -1
            while True:
                try:
                    state = manager.reconcile(DRIVER_NS, driver_labels, policy,
                                              converge=converge)
                except (BuildStateError, NotFoundError, StaleClusterViewError):
                    # transient cache view of an object mid-recreation;
                    # the reference requeues the reconcile on error
                    # (upgrade_state.go:128-131) — retry next round
                    rounds += 1
                    time.sleep(0.0005)
                    continue
                rounds += 1
                if mode == "anic":
                    # the in-flight communication jobs complete while the
                    # node waits (wait-for-jobs hook observes Succeeded)
                    for ns_ in state.nodes_in(
                            consts.UPGRADE_STATE_WAIT_FOR_JOBS_REQUIRED):
                        node_name = ns_.node["metadata"]["name"]
                        try:
                            sim.patch(
                                "v1", "Pod", f"comm-{node_name}",
                                {"status": {"phase": "Succeeded",
                                            "containerStatuses": [
                                                {"name": "allreduce",
                                                 "ready": False,
                                                 "restartCount": 0}]}},
                                "default",
                            )
                        except Exception:
                            pass
                # validation pods: run the real GPU check, then mark Ready
                for ns_ in state.nodes_in(consts.UPGRADE_STATE_VALIDATION_REQUIRED):
                    node_name = ns_.node["metadata"]["name"]
                    if gpu_validate:
                        validation_errs[node_name] = _run_gpu_validation(
                            device, mode=mode)
                    sim.patch(
                        "v1", "Pod", f"validator-{node_name}",
                        {"status": {"containerStatuses": [
                            {"name": "v", "ready": True, "restartCount": 0}]}},
                        DRIVER_NS,
                    )
                done = sum(
                    1 for n in client.list_nodes()
                    if n["metadata"]["labels"].get(state_key)
                    == consts.UPGRADE_STATE_DONE
                )
                if done == n_nodes:
                    # measurement integrity: completion must hold in the
                    # AUTHORITATIVE store, not just this client's (possibly
                    # stale) view — round-1's cached numbers broke early on
                    # the previous iteration's done labels still in cache
                    sim_done = sum(
                        1 for n in sim.list("v1", "Node")
                        if (n["metadata"].get("labels") or {}).get(state_key)
                        == consts.UPGRADE_STATE_DONE
                    )
                    if sim_done == n_nodes:
                        break
                    done = -1  # view was stale: keep reconciling
                if rounds > 200 * n_nodes:
                    raise RuntimeError(
                        f"upgrade did not converge after {rounds} rounds"
                    )
                if done == last_done and substrate != "inproc":
                    # waiting on async workers / informer propagation —
                    # yield instead of hammering the apiserver
                    time.sleep(0.0005)
                last_done = done
            elapsed = time.perf_counter() - t0
            ticks = registry.reconcile_duration.count
            if timed:
                tick_times.extend(registry.reconcile_duration.samples())
                wall_times.append(elapsed)
                ticks_per_upgrade.append(ticks)
                completed += 1
            manager.wait_idle()
            if collect_outputs and it == warmup + steps - 1:
                outputs = collect_step_outputs(sim, n_nodes, state_key,
                                               "newrev", validation_errs)
            ctrl.retarget({"metadata": {"uid": "-"}})
            cleanup()
            # iteration isolation: drain the previous cluster's DELETED
            # events out of the cache before re-creating same-named objects
            if substrate != "inproc":
                deadline = time.monotonic() + 30
                while time.monotonic() < deadline:
                    try:
                        if not client.list_nodes():
                            break
                    except Exception:
                        pass
                    time.sleep(0.001)
    finally:
        util.set_driver_name(prev_driver)
        CommonUpgradeManager.MAX_PARALLEL_NODE_OPS = prev_fanout
        close_substrate()

    return {
        "substrate": substrate,
        "outputs": outputs,
        "upgrades_completed": completed,
        "mean_wall_s": statistics.mean(wall_times) if wall_times else 0.0,
        "wall_times": wall_times,
        "reconcile_p50_ms": (
            statistics.median(tick_times) * 1000 if tick_times else 0.0
        ),
        "reconcile_p99_ms": (
            sorted(tick_times)[int(len(tick_times) * 0.99)] * 1000 if tick_times else 0.0
        ),
        "mean_ticks_per_upgrade": (
            statistics.mean(ticks_per_upgrade) if ticks_per_upgrade else 0.0
        ),
    }


# ---------------------------------------------------------------------------
# distributed entry point (driver contract)
# ---------------------------------------------------------------------------

def main():
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--nodes", type=int, default=8, help="simulated nodes per cluster")
    parser.add_argument("--max-parallel", type=int, default=2)
    parser.add_argument("--no-gpu-validate", action="store_true")
    parser.add_argument("--no-converge", action="store_true",
                        help="reference semantics: one state transition per reconcile tick")
    parser.add_argument("--mode", choices=["inplace", "requestor", "anic"],
                        default="inplace",
                        help="in-place node ops | maintenance-operator "
                             "delegation | NIC/xGMI driver path (config #4)")
    parser.add_argument("--substrate", choices=["cached", "http", "inproc"],
                        default="cached",
                        help="cached = informers->REST->HTTP apiserver "
                             "(production-shaped, HEADLINE); http = direct "
                             "REST; inproc = round-1 dict store")
    parser.add_argument("--no-secondary-substrates", action="store_true",
                        help="with --full: skip the reduced-step runs of the "
                             "other two substrates")
    parser.add_argument("--full", action="store_true",
                        help="after the timed steps, also run the comparison "
                             "measurements (reduced-step runs of the other "
                             "two substrates) and report them under "
                             "'substrates'")
    parser.add_argument("--dump-outputs", metavar="DIR", default=None,
                        help="write what the last timed step computed as "
                             "DIR/<name>.npy (float64, per node)")
    args = parser.parse_args()
    if args.steps < 1:
        parser.error("--steps must be at least 1")

    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    have_cuda = torch.cuda.is_available()
    gpu_validate = have_cuda and not args.no_gpu_validate

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        backend = "nccl" if have_cuda else "gloo"
        dist.init_process_group(backend=backend)
        if have_cuda:
            torch.cuda.set_device(local_rank)

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if have_cuda:
            torch.cuda.synchronize()

    converge = not args.no_converge
    # warmup (untimed) + timed section bracketed by barrier+sync on both sides
    run_rolling_upgrade_benchmark(
        n_nodes=args.nodes, steps=0, warmup=args.warmup,
        max_parallel=args.max_parallel, gpu_validate=gpu_validate,
        device=local_rank if have_cuda else 0, converge=converge,
        mode=args.mode, substrate=args.substrate,
    )
    barrier_sync()
    t0 = time.perf_counter()
    result = run_rolling_upgrade_benchmark(
        n_nodes=args.nodes, steps=args.steps, warmup=0,
        max_parallel=args.max_parallel, gpu_validate=gpu_validate,
        device=local_rank if have_cuda else 0, converge=converge,
        mode=args.mode, substrate=args.substrate,
        collect_outputs=bool(args.dump_outputs) and rank == 0,
    )
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if result["outputs"] is not None:
        import numpy as np

        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in result["outputs"].items():
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), arr)

    # --full: comparison runs of the non-headline substrates (reduced step
    # count, outside the timed region; rank 0 only)
    substrate_results = {args.substrate: {
        "mean_wall_s": result["mean_wall_s"],
        "reconcile_p50_ms": result["reconcile_p50_ms"],
        "steps": args.steps,
    }}
    if rank == 0 and args.full and not args.no_secondary_substrates:
        for other in ("cached", "http", "inproc"):
            if other == args.substrate:
                continue
            r = run_rolling_upgrade_benchmark(
                n_nodes=args.nodes, steps=min(3, args.steps), warmup=1,
                max_parallel=args.max_parallel, gpu_validate=False,
                converge=converge, mode=args.mode, substrate=other,
            )
            substrate_results[other] = {
                "mean_wall_s": r["mean_wall_s"],
                "reconcile_p50_ms": r["reconcile_p50_ms"],
                "steps": min(3, args.steps),
            }

    # MAX over ranks for time-like metrics
    if dist is not None:
        t = torch.tensor([elapsed, result["mean_wall_s"], result["reconcile_p50_ms"]],
                         dtype=torch.float64,
                         device="cuda" if have_cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, mean_wall_s, reconcile_p50_ms = t.tolist()
    else:
        mean_wall_s = result["mean_wall_s"]
        reconcile_p50_ms = result["reconcile_p50_ms"]

    if rank == 0:
        out = {
            "metric": "8-node rolling-upgrade wall-clock",
            "value": mean_wall_s,
            "unit": "s",
            "substrate": args.substrate,
            "substrates": substrate_results,
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": False,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic (synthetic amd.com/gpu pods; substrate="
                    f"{args.substrate}: "
                    + ("informer cache -> REST -> HTTP apiserver"
                       if args.substrate == "cached" else
                       "REST -> HTTP apiserver" if args.substrate == "http"
                       else "in-process store")
                    + "; reference publishes no baseline numbers)",
            "config": {
                "model": ("anic" if args.mode == "anic" else "amdgpu")
                + "-driver-rolling-upgrade",
                "substrate": args.substrate,
                "nodes_per_cluster": args.nodes,
                "maxParallelUpgrades": args.max_parallel,
                "maxUnavailable": "50%",
                "drain": True,
                "podDeletion": True,
                "gpu_pods_per_node": 2,
                "gpu_validation": gpu_validate,
                "converging_reconcile": converge,
                "mode": args.mode,
                "global_batch": args.nodes * int(os.environ.get("WORLD_SIZE", "1")),
                "parallelism": f"dp{world} (one independent simulated "
                               f"{args.nodes}-node cluster per rank)",
            },
            "reconcile_p50_ms": reconcile_p50_ms,
            "reconcile_p99_ms": result["reconcile_p99_ms"],
            "mean_ticks_per_upgrade": result["mean_ticks_per_upgrade"],
            "aggregate_node_upgrades_per_s": args.nodes * world / mean_wall_s
            if mean_wall_s else None,
        }
        print(json.dumps(out))

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
