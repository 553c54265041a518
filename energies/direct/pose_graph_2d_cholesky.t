-- 2-D pose graph with H = J^T J formed explicitly and solved directly:
-- normal_matrix/pose_graph_2d_explicit.t plus LinearSolver("cholesky"). Each Step fills H (+ LM's
-- diagonal) into dense tiles, factors it H = L L^T and takes the exact Gauss-Newton / LM step
-- instead of lIterations of PCG. Same problemparams, same energy. Runs on generated kernels.
local N, E = Dim("N", 0), Dim("E", 1)

local w_anchor = Param("w_anchor", float, 0)
local P  = Unknown("P", opt_float3, {N}, 1)    -- x, y, theta
local P0 = Array("P0", opt_float3, {N}, 2)
local A  = Array("A", opt_float, {N}, 3)       -- 1 on anchored poses, 0 elsewhere
local Z  = Array("Z", opt_float3, {E}, 4)      -- measured dx, dy, dtheta
local U0 = Array("U0", opt_float3, {E}, 5)
local U1 = Array("U1", opt_float3, {E}, 6)
local G  = Graph("G", {E}, "i", {N}, 7, "j", {N}, 8, "e", {E}, 9)
UsePreconditioner(true)
NormalMatrix("explicit")
LinearSolver("cholesky")

Energy(w_anchor * A(0) * (P(0) - P0(0)))

local pi, pj = P(G.i), P(G.j)
local z, u0, u1 = Z(G.e), U0(G.e), U1(G.e)
local dx, dy = pj(0) - pi(0), pj(1) - pi(1)
local c, s = cos(pi(2)), sin(pi(2))
local e0 = c * dx + s * dy - z(0)
local e1 = c * dy - s * dx - z(1)
local d  = pj(2) - pi(2) - z(2)
local e2 = atan2(sin(d), cos(d))
Energy(u0(0) * e0 + u0(1) * e1 + u0(2) * e2)
Energy(u1(0) * e1 + u1(1) * e2)
Energy(u1(2) * e2)
