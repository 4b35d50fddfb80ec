------------------------------ MODULE parity_view ------------------------------
(* The guards read only the parity of x, and a step flips it: VIEW <<x % 2, pc>> — a view with a scalar EXPRESSION — is a congruence of a
   model whose x grows without bound. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm parity_view
variables x = 0;

process P \in 0..1
begin
  a: await x % 2 = self;
     x := x + 1;
  b: either goto a or skip end either;
end process

end algorithm *)

View == <<x % 2, pc>>
=============================================================================
