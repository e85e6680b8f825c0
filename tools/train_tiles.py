"""Print the Winograd tile of every layer of the RFBNet-300 bs-32 training runtime: forward, data gradient, weight-gradient route."""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'context-transformer_amd')]

from ctdet import synth  # noqa: E402
from models.RFB_Net_vgg import build_net  # noqa: E402

net = build_net(types.SimpleNamespace(method='ours', phase=1, setting='transfer'), 300, 20)
net.load_state_dict(synth.fill_state_dict(net.state_dict()))
net = net.cuda().train()
net.device = 'cuda'
trt = net.train_runtime(32)
for st in trt.plan.steps:
    if st.kind == 'conv':
        s = trt.state[st.name]          # train_engine.LayerState
        if s.fwd.rt.get('wino') or s.dgrad_tile:
            print(st.name, st.cin, st.cout, st.h, 'fwd', s.fwd.rt.get('wino'), 'dgrad', s.dgrad_tile, 'wgrad', s.wgrad_route.name)
