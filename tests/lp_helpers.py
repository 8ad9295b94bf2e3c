"""Shared by the KAO-LP parity tests (test_gpu_lp.py, test_gpu_lp_paths.py): drifted synthetic topics in both classes, and the
per-iterate rule the device trace is held to against the scalar restatement."""
import numpy as np


def otopic(ko, pt):
    """product Topic -> oracle Topic"""
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                    bounds_override=dict(pt.bounds_override))


def drift_topic(ko, B, R, P, dseed=1, rf=3, new_rf=None):
    """B brokers on R racks, P partitions of RF `rf` (then `new_rf`, if given) after a 20 % drift: (product Topic, oracle Topic)"""
    from kafka_assignment_optimizer_amd import synthetic as sy
    pt = sy.drift(sy.make_cluster(B, R, 1, P, rf, [], [], new_rf=new_rf), 0.2, dseed)[0]
    return pt, otopic(ko, pt)


def trace_close(dev, ref, rel=1e-7):
    """mu, primal and dual objective of every iterate agree to `rel` while mu >= 1e-6 (afterwards both are at the optimum and
    the last digits are rounding); the iteration counts differ by at most one."""
    assert abs(len(dev) - len(ref)) <= 1, (len(dev), len(ref))
    for a, b in zip(dev, ref):
        if b[0] < 1e-6:
            break
        assert abs(a[0] - b[0]) <= rel * b[0], (a, b)
        assert abs(a[1] - b[1]) <= rel * max(1.0, abs(b[1])) and abs(a[2] - b[2]) <= rel * max(1.0, abs(b[2])), (a, b)
